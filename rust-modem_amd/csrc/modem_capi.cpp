// rust-modem_amd/csrc/modem_capi.cpp — implementation of include/modem_hip.h.
//
// Host side of the drop-in boundary: phasor LUT builders (the memoryless DigitalPhasor
// plugins evaluated once per symbol value, same expressions and rounding as the reference),
// RRC tap generation, and the streaming TX / RX / FIR handles that own device state and
// launch the kernels of modem_kernels.hip. Built with -ffp-contract=off so host float
// expressions round like rustc's.
#include "../../include/modem_hip.h"
#include "modem_internal.h"
#include "modem_fec_math.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr float kPi = 3.14159265358979323846f;   // std::f32::consts::PI

struct DeviceGuard {   // scoped hipSetDevice (no call when the device is already current)
    int old = -1;
    bool ok = false, set = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&old) != hipSuccess) { (void)hipGetLastError(); old = -1; }
        if (old == dev) { ok = true; return; }
        ok = hipSetDevice(dev) == hipSuccess;
        set = ok;
        if (!ok) (void)hipGetLastError();
    }
    ~DeviceGuard() { if (set && old >= 0) (void)hipSetDevice(old); }
};

bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// Device memory of a GPU other than `dev` (managed memory is reachable from every device).
// A handle's kernels run on its own device: such a buffer would be read over the fabric or
// fault, so the entry points refuse it (the reference has one address space, no counterpart).
bool foreign_ptr(const void* p, int dev) {
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice && a.device != dev;
}

// Both facts from one attribute query (the per-call host cost of a process() is mostly these
// queries): host memory (staged), device memory the handle's kernels can use, or another
// GPU's memory (refused).
enum PtrKind { PTR_HOST = 0, PTR_DEVICE = 1, PTR_FOREIGN = 2 };
PtrKind ptr_kind(const void* p, int dev) {
    if (!p) return PTR_HOST;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return PTR_HOST; }
    if (a.type == hipMemoryTypeManaged) return PTR_DEVICE;
    if (a.type != hipMemoryTypeDevice) return PTR_HOST;
    return a.device == dev ? PTR_DEVICE : PTR_FOREIGN;
}

#define HIP_TRY(expr)                                                              \
    do {                                                                           \
        if ((expr) != hipSuccess) { (void)hipGetLastError(); return MODEM_ERR_HIP; } \
    } while (0)

template <typename T>
modem_status dalloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    if (hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return MODEM_ERR_ALLOC;
    }
    if (hipMemset(*p, 0, count * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return MODEM_ERR_HIP; }
    return MODEM_OK;
}

// Growable device staging buffer for host-pointer I/O.
struct Stage {
    void* p = nullptr;
    size_t cap = 0;
    modem_status ensure(size_t bytes) {
        if (bytes <= cap) return MODEM_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return MODEM_ERR_ALLOC; }
        cap = bytes;
        return MODEM_OK;
    }
    ~Stage() { if (p) (void)hipFree(p); }
};

// Growable device workspace of a handle's device-only path (include/modem_hip.h, "Streams").
// Growing never frees: hipFree waits for the whole device, which a call documented as asynchronous
// must not do, and kernels already queued may still use the old buffer. A buffer that was outgrown
// is retired and lives until the handle is destroyed; the capacity at least doubles each time, so
// the retired buffers together stay below the live one.
struct Workspace {
    void* p = nullptr;
    size_t cap = 0;
    std::vector<void*> retired;
    modem_status ensure(size_t bytes) {
        if (bytes <= cap) return MODEM_OK;
        const size_t want = std::max(bytes, 2 * cap);
        void* q = nullptr;
        if (hipMalloc(&q, want) != hipSuccess) { (void)hipGetLastError(); return MODEM_ERR_ALLOC; }
        if (p) retired.push_back(p);
        p = q;
        cap = want;
        return MODEM_OK;
    }
    ~Workspace() {
        if (p) (void)hipFree(p);
        for (void* r : retired) (void)hipFree(r);
    }
};

bool device_ok(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return false; }
    return device >= 0 && device < n;
}

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

modem_status phasor_bps(const modem_phasor_desc* d, uint32_t* bps) {
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

bool phasor_scanned(int kind) {          // phase carried from symbol to symbol (tx_scan)
    return kind == MODEM_PHASOR_DMPSK || kind == MODEM_PHASOR_MFSK || kind == MODEM_PHASOR_BFSK;
}
bool phasor_sample_dependent(int kind) {
    return kind == MODEM_PHASOR_DCQPSK || kind == MODEM_PHASOR_CPFSK || kind == MODEM_PHASOR_MSK ||
           phasor_scanned(kind);
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

// =====================================================================================
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

int32_t modem_abi_version(void) { return MODEM_HIP_ABI_VERSION; }

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
    if (n && (!out || !is_device_ptr(out) || foreign_ptr(out, device))) return MODEM_ERR_INVALID_ARG;
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

// ------------------------------------------------------------------------------ TX ----
struct modem_tx {
    int device = 0;
    uint32_t bps = 0, sps = 0, ntaps = 0, K = 1;
    float w = 0.f;
    uint64_t sample = 0;
    int dtype = 0, out_mode = 0;
    float2* d_lut = nullptr;
    float* d_taps = nullptr;
    float* d_taps_q = nullptr;      // Q-rail taps when q_offset != 0
    uint32_t q_offset = 0;
    int ph_kind = 0;                // sample-dependent phasor (tx_phasor), else 0
    float ph_amp = 0.f, ph_freq = 0.f, ph_shift = 0.f, ph_max = 0.f;
    int ph_spb = 0, ph_map = 0;
    Workspace scan_stage;           // per-symbol states of the scanned phasors
    size_t scan_n = 0;              // symbols of the last call, in scan_stage (modem_tx_scan_states)
    int scan_path = 0;              // how the last call scanned them (modem_tx_scan_path)
    Workspace batch_params;         // a scan batch's parameter blocks, when this is its first handle
    float2* d_hist[2] = {nullptr, nullptr};
    uint8_t* d_carry[2] = {nullptr, nullptr};
    int hcur = 0, ccur = 0, ncarry = 0;
    int mfma_ksteps = 0;            // > 0: FIR on the matrix cores (tx_mfma)
    float* d_bfrag = nullptr;       // its split-f16 per-lane B fragments (modem_internal.h)
    std::vector<_Float16> bfrag_host;   // the same, on the host (batch compatibility check)
    float* d_luth = nullptr;        // its split-f16 LUT (re_hi, re_lo, im_hi, im_lo per entry)
    int lut_scale_exp = 0, tap_scale_exp = 0;
    int levels = 0;                 // integer-level LUT (see TxParams)
    float level_inv = 0.0f;
    uint64_t symbols = 0;           // symbols emitted so far (row-block alignment)
    Stage bits_stage, out_stage;
    ~modem_tx() {
        DeviceGuard g(device);
        for (void* p : {(void*)d_lut, (void*)d_taps, (void*)d_taps_q, (void*)d_hist[0], (void*)d_hist[1],
                        (void*)d_carry[0], (void*)d_carry[1], (void*)d_bfrag, (void*)d_luth})
            if (p) (void)hipFree(p);
    }
};

static size_t tx_sample_bytes(const modem_tx* h) {
    const size_t v = h->dtype == MODEM_DTYPE_F16 ? 2 : 4;
    return h->out_mode == MODEM_OUT_REAL ? v : 2 * v;
}

modem_status modem_tx_create(const modem_tx_desc* d, int device, modem_tx** out) {
    if (!d || !out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (d->bits_per_symbol < 1 || d->bits_per_symbol > 8) return MODEM_ERR_INVALID_ARG;
    if (d->samples_per_symbol < 1) return MODEM_ERR_INVALID_ARG;   // SymbolClock % 0 panics (data.rs:29)
    if (d->ntaps > (uint32_t)mk::kMaxTaps || (d->ntaps && !d->taps)) return MODEM_ERR_INVALID_ARG;
    if (d->dtype != MODEM_DTYPE_F32 && d->dtype != MODEM_DTYPE_F16) return MODEM_ERR_INVALID_ARG;
    if (d->out_mode < MODEM_OUT_IQ_MIXED || d->out_mode > MODEM_OUT_REAL) return MODEM_ERR_INVALID_ARG;
    // EvenOddOffset::new asserts bits_per_symbol == 2 and an even samples_per_symbol (data.rs:91-92)
    if (d->q_offset != 0 && (d->bits_per_symbol != 2 || d->samples_per_symbol % 2 != 0 ||
                             d->q_offset != d->samples_per_symbol / 2))
        return MODEM_ERR_INVALID_ARG;
    // Sample-dependent phasors (tx_phasor): sample-and-hold only; the LUT is built here.
    const modem_phasor_desc* pd = d->phasor;
    std::vector<float> plut;
    if (pd) {
        uint32_t pbps = 0;
        if (!phasor_sample_dependent(pd->kind) || phasor_bps(pd, &pbps) != MODEM_OK ||
            pbps != d->bits_per_symbol)
            return MODEM_ERR_INVALID_ARG;
        if (d->ntaps != 0) return MODEM_ERR_UNSUPPORTED;
        if (pd->kind == MODEM_PHASOR_MSK && (pd->samples_per_symbol == 0 || pd->samples_per_symbol % 2))
            return MODEM_ERR_INVALID_ARG;                                   // msk.rs:14
        if (d->q_offset && pd->kind != MODEM_PHASOR_MSK) return MODEM_ERR_UNSUPPORTED;
        if (pd->kind == MODEM_PHASOR_DCQPSK) {                              // dcqpsk.rs:23-36
            const float map[4] = {0.0f, kPi / 2.0f, 3.0f * kPi / 2.0f, kPi};
            for (int parity = 0; parity < 2; ++parity)     // even symbol count -> term + pi/4
                for (int k = 0; k < 4; ++k) {
                    const float term = parity == 0 ? map[k] + kPi / 4.0f : map[k];
                    plut.push_back(pd->amplitude * std::cos(term));         // :46-52
                    plut.push_back(pd->amplitude * std::sin(term));
                }
        }
    } else if (!d->lut) {
        return MODEM_ERR_INVALID_ARG;
    }
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_tx* h = new (std::nothrow) modem_tx;
    if (!h) return MODEM_ERR_ALLOC;
    h->device = device;
    if (pd) {
        h->ph_kind = pd->kind;
        h->ph_amp = pd->amplitude;
        h->ph_freq = pd->freq;
        h->ph_spb = (int)(pd->samples_per_symbol / 2);
        h->ph_shift = pd->shift;
        h->ph_map = pd->mfsk_map ? 1 : 0;
        h->ph_max = (float)((1u << d->bits_per_symbol) - 1u);                 // max_symbol, util.rs:13-15
    }
    h->bps = d->bits_per_symbol;
    h->sps = d->samples_per_symbol;
    h->ntaps = d->ntaps;
    h->w = d->sample_freq;
    h->sample = d->s0;
    h->dtype = d->dtype;
    h->out_mode = d->out_mode;
    h->q_offset = d->q_offset;
    // ntaps == 0: the reference's sample-and-hold == zero-stuffing + sps unit taps. A Q offset
    // D delays the Q rail: its taps are h[j - D] (length L + D).
    const uint32_t L = d->ntaps ? d->ntaps : d->samples_per_symbol;
    const uint32_t D = d->q_offset;
    h->K = (L + D + h->sps - 1) / h->sps;
    // pp[t*sps + p] = h[p + sps*t]; padded by mk::kTapPad steps of zeros so the kernels'
    // look-ahead tap loads stay in bounds.
    std::vector<float> pp((size_t)(h->K + mk::kTapPad) * h->sps, 0.0f), pq;
    auto tap = [&](uint32_t j) { return d->ntaps ? d->taps[j] : 1.0f; };
    for (uint32_t j = 0; j < L; ++j) pp[(size_t)(j / h->sps) * h->sps + j % h->sps] = tap(j);
    if (D) {
        pq.assign(pp.size(), 0.0f);
        for (uint32_t j = 0; j < L; ++j) pq[(size_t)((j + D) / h->sps) * h->sps + (j + D) % h->sps] = tap(j);
    }
    modem_status st;
    const size_t nl = pd ? std::max<size_t>(1, plut.size() / 2) : (size_t)1 << h->bps;
    const float* lut_src = pd ? plut.data() : d->lut;
    if ((st = dalloc(&h->d_lut, nl)) || (st = dalloc(&h->d_taps, pp.size())) ||
        (st = dalloc(&h->d_hist[0], h->K)) || (st = dalloc(&h->d_hist[1], h->K)) ||
        (st = dalloc(&h->d_carry[0], 8)) || (st = dalloc(&h->d_carry[1], 8)) ||
        (D && (st = dalloc(&h->d_taps_q, pq.size())))) {
        delete h;
        return st;
    }
    if ((lut_src && hipMemcpy(h->d_lut, lut_src, nl * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(h->d_taps, pp.data(), pp.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        (D && hipMemcpy(h->d_taps_q, pq.data(), pq.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)) {
        (void)hipGetLastError();
        delete h;
        return MODEM_ERR_HIP;
    }
    // Sample-and-hold EvenOddOffset: before the first Q tick the phasor sees cur = [b0, 0]
    // (data.rs:84), i.e. the Q value of symbol index 0; it enters as the history symbol that
    // the delayed Q rail reads for n < D (its I value meets zero taps).
    // DMPSK starts from its phase (dmpsk.rs:20); MFSK / BFSK from zeros (mfsk.rs:55-56, bfsk.rs:16-17)
    if (pd && pd->kind == MODEM_PHASOR_DMPSK) {
        const float2 st0 = make_float2(pd->phase, 0.0f);
        if (hipMemcpy(h->d_hist[0], &st0, sizeof st0, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            delete h;
            return MODEM_ERR_HIP;
        }
    }
    if (D && d->ntaps == 0 && !pd &&
        hipMemcpy(h->d_hist[0] + (h->K - 2), d->lut, sizeof(float2), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        delete h;
        return MODEM_ERR_HIP;
    }
    // FIR path: the matrix pipe when the (sps, K) shape has an instantiated kernel, unless
    // MODEM_HIP_FIR=valu forces the packed-VALU kernel (both are parity-tested).
    const char* env = std::getenv("MODEM_HIP_FIR");
    const bool force_valu = env && std::strcmp(env, "valu") == 0;
    // Sample-and-hold (no taps) stays on the VALU kernels, which reproduce it bit for bit.
    h->mfma_ksteps = (force_valu || d->ntaps == 0 || D || pd) ? 0 : mk::tx_mfma_ksteps((int)h->sps, (int)h->K);
    if (h->mfma_ksteps > 0) {
        // Split-f16 operands of tx_mfma (modem_tx.hip). Exact power-of-two scales put the
        // maxima of the LUT and of the taps in [2^14, 2^15); both are split hi + lo =
        // rn_f16(v) + rn_f16(v - hi).
        auto scale_exp = [](float mx) {   // 0 inside [2^-3, 2^15), else into [2^14, 2^15)
            int e = 0;
            if (!(mx > 0.0f) || !std::isfinite(mx) || (mx >= 0.125f && mx < 32768.0f)) return 0;
            std::frexp(mx, &e);
            return 15 - e;
        };
        auto split = [](float v, _Float16& hi, _Float16& lo) { hi = (_Float16)v; lo = (_Float16)(v - (float)hi); };
        float lmax = 0.0f, tmax = 0.0f;
        for (size_t k = 0; k < 2 * nl; ++k) lmax = std::max(lmax, std::fabs(d->lut[k]));
        for (uint32_t k = 0; k < d->ntaps; ++k) tmax = std::max(tmax, std::fabs(d->taps[k]));
        // Integer levels: every component v = q * s, q an integer with |q| <= 2048 (exact f16),
        // s the smallest nonzero |component|. Then A = q exactly and s moves into the taps.
        double smin = 0.0;
        for (size_t k = 0; k < 2 * nl; ++k) {
            const double a = std::fabs((double)d->lut[k]);
            if (a > 0.0 && (smin == 0.0 || a < smin)) smin = a;
        }
        bool levels = smin > 0.0;
        for (size_t k = 0; levels && k < 2 * nl; ++k) {
            const double q = (double)d->lut[k] / smin, r = std::nearbyint(q);
            levels = std::fabs(r) <= 2048.0 && std::fabs(q - r) <= 1e-6 * std::max(1.0, std::fabs(q));
        }
        h->levels = levels ? 1 : 0;
        h->level_inv = levels ? (float)(1.0 / smin) : 0.0f;
        const double tscale = levels ? smin : 1.0;           // folded into the taps
        tmax = (float)(tmax * tscale);
        h->lut_scale_exp = levels ? 0 : scale_exp(lmax);
        h->tap_scale_exp = scale_exp(tmax);
        std::vector<_Float16> lh(4 * nl);
        for (size_t k = 0; k < nl; ++k) {
            if (levels) {
                lh[4 * k] = (_Float16)std::nearbyint((double)d->lut[2 * k] / smin);
                lh[4 * k + 2] = (_Float16)std::nearbyint((double)d->lut[2 * k + 1] / smin);
                lh[4 * k + 1] = lh[4 * k + 3] = (_Float16)0.0f;
                continue;
            }
            split(std::ldexp(d->lut[2 * k], h->lut_scale_exp), lh[4 * k], lh[4 * k + 1]);
            split(std::ldexp(d->lut[2 * k + 1], h->lut_scale_exp), lh[4 * k + 2], lh[4 * k + 3]);
        }
        // B[o][j] = h[p + sps*(c + PRE - o)], j = sps*c + p: lane l holds, for k-step s, the 8
        // window offsets o = 32s + 8(l >> 4) + jj of column j = l & 15, hi then lo.
        const int nks = h->mfma_ksteps, sps = (int)h->sps, SB = 16 / sps, PRE = 32 * nks - SB;
        std::vector<_Float16> bf((size_t)nks * 2 * 64 * 8, (_Float16)0.0f);
        for (int s2 = 0; s2 < nks; ++s2)
            for (int l = 0; l < 64; ++l)
                for (int jj = 0; jj < 8; ++jj) {
                    const int o = 32 * s2 + 8 * (l >> 4) + jj, j = l & 15, c = j / sps, ph = j % sps;
                    const int t = c + PRE - o;
                    const float v = (t >= 0 && t < (int)h->K)
                        ? std::ldexp((float)((double)pp[(size_t)t * sps + ph] * tscale), h->tap_scale_exp) : 0.0f;
                    split(v, bf[(((size_t)s2 * 2) * 64 + l) * 8 + jj], bf[(((size_t)s2 * 2 + 1) * 64 + l) * 8 + jj]);
                }
        const size_t nb = (bf.size() * sizeof(_Float16) + sizeof(float) - 1) / sizeof(float);
        const size_t nlh = (lh.size() * sizeof(_Float16) + sizeof(float) - 1) / sizeof(float);
        if ((st = dalloc(&h->d_bfrag, nb)) || (st = dalloc(&h->d_luth, nlh))) { delete h; return st; }
        h->bfrag_host = bf;
        if (hipMemcpy(h->d_bfrag, bf.data(), bf.size() * sizeof(_Float16), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_luth, lh.data(), lh.size() * sizeof(_Float16), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            delete h;
            return MODEM_ERR_HIP;
        }
    }
    *out = h;
    return MODEM_OK;
}

// Non-temporal TX stores for large launches. A launch writing more than the Infinity Cache
// holds (256 MiB on MI355X) streams its samples through it to HBM anyway, and its dirty lines
// are then written back while the RX reads the buffer. Such a launch (over 192 MiB: C5, 512
// MiB) stores its samples non-temporally, straight to HBM. In-tree A/B of this host switch
// (profiles/r03_tx_nt.txt, bench legs): C5 chain 280.9 -> 268.5 us, TX alone 135 -> 109 us,
// the RX in the chain 145.5 -> 159.5 us (it now reads everything from HBM); C4 chain 121 ->
// 116.6 us. (The earlier compile-time all-NT build measured C5 chain 273.4 -> 257.9 us on
// another box; keeping the last 128 MiB cacheable, 261.4.) A single-channel launch of at most
// the Infinity Cache's size (C5 f16: 256 MiB) stores only its first half non-temporally: the
// RX, walking its tiles top-down, then finds the second half in the cache (chain 182.6 ->
// 178.3-179.2 us, profiles/r04_tx_nt.txt; the same split for C5 f32 and for C4's 8-channel
// batch was slower: 265 vs 261 us, 125.8 vs 120 us). Smaller launches (C3: 128 MiB, whose RX
// re-reads it from the cache) keep the default policy. MODEM_TX_NT=0 turns it off (A/B),
// MODEM_TX_NT=1 stores every large launch's samples non-temporally.
// `launch_bytes`: the whole launch's output (every channel of a batch); returns nt_below.
static int64_t tx_nt_below(int64_t nsamp, uint64_t launch_bytes, bool single) {
    static const int mode = [] { const char* e = std::getenv("MODEM_TX_NT"); return e ? std::atoi(e) : 2; }();
    constexpr uint64_t kMin = 192ull << 20, kCache = 256ull << 20;
    if (mode == 0 || launch_bytes <= kMin || nsamp <= 0) return 0;
    // the cacheable second half pays only because the RX reads it first (mk::kRxTilesTopDown)
    return mode == 2 && single && mk::kRxTilesTopDown && launch_bytes <= kCache ? nsamp / 2 : nsamp;
}

// Kernel parameters of one TX call on device buffers (dbits, dout); see tx_run.
static void tx_fill(const modem_tx* h, const uint8_t* dbits, size_t nbits, bool flush, void* dout,
                    int64_t nsym, int ncarry_new, size_t nsamp, mk::TxParams& p) {
    p.bits = dbits;
    p.carry = h->d_carry[h->ccur];
    p.carry_new = h->d_carry[h->ccur ^ 1];
    p.hist = h->d_hist[h->hcur];
    p.hist_new = h->d_hist[h->hcur ^ 1];
    p.lut = h->d_lut;
    p.taps = h->d_taps;
    p.taps_q = h->d_taps_q;
    p.out = dout;
    p.nt_below = tx_nt_below((int64_t)nsamp, (uint64_t)nsamp * tx_sample_bytes(h), true);
    p.s0 = h->sample;
    p.nsym = nsym;
    p.nsym_valid = flush ? 0 : nsym;
    p.nbits = (int64_t)nbits;
    p.ncarry = h->ncarry;
    p.ncarry_new = ncarry_new;
    p.update_carry = flush ? 0 : 1;
    p.bps = (int)h->bps;
    p.sps = (int)h->sps;
    p.K = (int)h->K;
    p.fast_bits = (h->ncarry == 0 && (h->bps == 1 || h->bps == 2 || h->bps == 4 || h->bps == 8) &&
                   ((uintptr_t)dbits % h->bps) == 0) ? 1 : 0;
    p.exact_idx = (h->sample + nsamp) <= (1ull << 53) ? 1 : 0;
    p.idx46 = (h->sample + nsamp + 256) < (1ull << 46) ? 1 : 0;
    p.w = h->w;
    p.lut_h = h->d_luth;
    p.lut_scale_exp = h->lut_scale_exp;
    p.tap_scale_exp = h->tap_scale_exp;
    p.levels = h->levels;
    p.level_inv = h->level_inv;
    const uint32_t sb = (h->sps <= 16 && 16 % h->sps == 0) ? 16 / h->sps : 1;   // symbols per row-block
    p.lead = (int)(h->symbols % sb);
    p.ph_kind = h->ph_kind;
    p.sym0 = h->symbols;
    p.ph_amp = h->ph_amp;
    p.ph_freq = h->ph_freq;
    p.ph_spb = h->ph_spb;
    p.q_off = (int)h->q_offset;
    p.ph_shift = h->ph_shift;
    p.ph_map = h->ph_map;
    p.ph_max = h->ph_max;
}

// The handle's state after a TX call (the kernel wrote the other history / carry buffers).
static void tx_advance(modem_tx* h, bool flush, int64_t nsym, int ncarry_new, size_t nsamp) {
    h->hcur ^= 1;
    if (!flush) { h->ccur ^= 1; h->ncarry = ncarry_new; }
    h->sample += nsamp;
    h->symbols += (uint64_t)nsym;
}

// The kernel launch of one TX call on device buffers and the handle's state update.
static modem_status tx_launch(modem_tx* h, const uint8_t* dbits, size_t nbits, bool flush, void* dout, int64_t nsym,
                              int ncarry_new, size_t nsamp, hipStream_t s) {
    modem_status st;
    mk::TxParams p{};
    tx_fill(h, dbits, nbits, flush, dout, nsym, ncarry_new, nsamp, p);
    p.scan = nullptr;
    if (phasor_scanned(h->ph_kind)) {
        h->scan_n = 0;                  // the stage is rewritten (or regrown): no states until this call is queued
        // (regrown without a free: the previous call's kernels may still be queued on its buffer)
        if ((st = h->scan_stage.ensure((size_t)std::max<int64_t>(nsym, 1) * sizeof(float2)))) return st;
        p.scan = static_cast<float2*>(h->scan_stage.p);
    }
    if (h->ph_kind)
        HIP_TRY(mk::launch_tx_phasor(p, h->dtype, h->out_mode, s));
    else if (h->mfma_ksteps > 0)
        HIP_TRY(mk::launch_tx_mfma(p, (int)h->sps, h->mfma_ksteps, h->d_bfrag, h->dtype, h->out_mode, s));
    else
        HIP_TRY(mk::launch_tx(p, (int)h->sps, h->dtype, h->out_mode, s));
    tx_advance(h, flush, nsym, ncarry_new, nsamp);
    if (p.scan) { h->scan_n = (size_t)nsym; h->scan_path = 1; }
    return MODEM_OK;
}

static modem_status tx_run(modem_tx* h, const uint8_t* bits, size_t nbits, bool flush, void* out,
                           size_t cap, size_t* produced, hipStream_t s) {
    if (!h || !produced || (nbits && !bits)) return MODEM_ERR_INVALID_ARG;
    *produced = 0;
    const uint64_t total = (uint64_t)h->ncarry + nbits;
    const int64_t nsym = flush ? (int64_t)((h->ntaps ? h->ntaps - 1 + h->q_offset : 0) + h->sps - 1) / h->sps
                               : (int64_t)(total / h->bps);
    const int ncarry_new = flush ? h->ncarry : (int)(total - (uint64_t)nsym * h->bps);
    const size_t nsamp = (size_t)nsym * h->sps;
    if (nsamp > cap) return MODEM_ERR_CAPACITY;
    if (nsamp && !out) return MODEM_ERR_INVALID_ARG;
    const PtrKind kb = nbits ? ptr_kind(bits, h->device) : PTR_DEVICE;
    const PtrKind ko = nsamp ? ptr_kind(out, h->device) : PTR_DEVICE;
    if (kb == PTR_FOREIGN || ko == PTR_FOREIGN) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    const uint8_t* dbits = bits;
    if (kb == PTR_HOST) {
        if ((st = h->bits_stage.ensure(nbits))) return st;
        HIP_TRY(hipMemcpyAsync(h->bits_stage.p, bits, nbits, hipMemcpyHostToDevice, s));
        dbits = static_cast<const uint8_t*>(h->bits_stage.p);
    }
    const bool host_out = ko == PTR_HOST;
    void* dout = out;
    if (host_out) {
        if ((st = h->out_stage.ensure(nsamp * tx_sample_bytes(h)))) return st;
        dout = h->out_stage.p;
    }
    if ((st = tx_launch(h, dbits, nbits, flush, dout, nsym, ncarry_new, nsamp, s))) return st;
    if (host_out) {
        HIP_TRY(hipMemcpyAsync(out, dout, nsamp * tx_sample_bytes(h), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    } else if (nbits && dbits != bits) {
        HIP_TRY(hipStreamSynchronize(s));   // host bits staged: keep the caller's view simple
    }
    *produced = nsamp;
    return MODEM_OK;
}

modem_status modem_tx_process(modem_tx* h, const uint8_t* bits, size_t nbits, void* out, size_t cap,
                              size_t* produced, void* stream) {
    return tx_run(h, bits, nbits, false, out, cap, produced, (hipStream_t)stream);
}
modem_status modem_tx_flush(modem_tx* h, void* out, size_t cap, size_t* produced, void* stream) {
    return tx_run(h, nullptr, 0, true, out, cap, produced, (hipStream_t)stream);
}
// Channels of one scanned phasor kind (DMPSK / MFSK / BFSK; modem_tx_process_batch): their serial
// symbol-state scans run as one launch, one lane per channel (tx_scan_batch: each channel's
// states bit for bit those of its single call), then each channel's sample kernel. Every buffer is
// device memory; the handles are distinct and share a device.
static modem_status tx_scan_batch_run(modem_tx* const* hs, size_t nch, const uint8_t* const* bits,
                                      const size_t* nbits, void* const* outs, const size_t* caps, size_t* produced,
                                      hipStream_t s) {
    std::vector<int64_t> nsym(nch);
    std::vector<int> ncarry_new(nch);
    for (size_t c = 0; c < nch; ++c) {        // every channel's size first: an error leaves the handles untouched
        const modem_tx* h = hs[c];
        const uint64_t total = (uint64_t)h->ncarry + nbits[c];
        nsym[c] = (int64_t)(total / h->bps);
        ncarry_new[c] = (int)(total - (uint64_t)nsym[c] * h->bps);
        if ((size_t)nsym[c] * h->sps > caps[c]) return MODEM_ERR_CAPACITY;
    }
    DeviceGuard g(hs[0]->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    std::vector<mk::TxParams> ps(nch);
    for (size_t c = 0; c < nch; ++c) {
        modem_tx* h = hs[c];
        h->scan_n = 0;
        if ((st = h->scan_stage.ensure((size_t)std::max<int64_t>(nsym[c], 1) * sizeof(float2)))) return st;
        tx_fill(h, bits[c], nbits[c], false, outs[c], nsym[c], ncarry_new[c], (size_t)nsym[c] * h->sps, ps[c]);
        ps[c].scan = static_cast<float2*>(h->scan_stage.p);
    }
    if ((st = hs[0]->batch_params.ensure(nch * sizeof(mk::TxParams)))) return st;
    // (from pageable host memory: synchronous, so `ps` may go when the call returns)
    HIP_TRY(hipMemcpyAsync(hs[0]->batch_params.p, ps.data(), nch * sizeof(mk::TxParams), hipMemcpyHostToDevice, s));
    HIP_TRY(mk::launch_tx_scan_batch(static_cast<const mk::TxParams*>(hs[0]->batch_params.p), (int)nch,
                                      hs[0]->ph_kind, s));
    for (size_t c = 0; c < nch; ++c) {
        modem_tx* h = hs[c];
        HIP_TRY(mk::launch_tx_phasor(ps[c], h->dtype, h->out_mode, s, true));
        tx_advance(h, false, nsym[c], ncarry_new[c], (size_t)nsym[c] * h->sps);
        h->scan_n = (size_t)nsym[c];
        h->scan_path = 2;
        produced[c] = (size_t)nsym[c] * h->sps;
    }
    return MODEM_OK;
}

// One launch for several channels (independent channel streams). Equivalent to
// modem_tx_process(hs[c], bits[c], nbits[c], outs[c], caps[c], &produced[c], stream) for
// c = 0 .. nch-1 in order; fused into one launch per kBatchMax channels when every handle
// shares the matrix-core configuration (sps, taps, bps, f32/f16 mixed I/Q output, device)
// and all buffers are device memory, otherwise run one call at a time.
modem_status modem_tx_process_batch(modem_tx* const* hs, size_t nch, const uint8_t* const* bits,
                                    const size_t* nbits, void* const* outs, const size_t* caps,
                                    size_t* produced, void* stream) {
    if (nch == 0) return MODEM_OK;
    if (!hs || !bits || !nbits || !outs || !caps || !produced) return MODEM_ERR_INVALID_ARG;
    const hipStream_t s = (hipStream_t)stream;
    for (size_t c = 0; c < nch; ++c)    // an error leaves every handle untouched
        if (hs[c] && ((nbits[c] && foreign_ptr(bits[c], hs[c]->device)) || foreign_ptr(outs[c], hs[c]->device)))
            return MODEM_ERR_INVALID_ARG;
    bool scan = nch >= 2 && hs[0] != nullptr && phasor_scanned(hs[0]->ph_kind);
    for (size_t c = 0; scan && c < nch; ++c) {
        const modem_tx* h = hs[c];
        // (a channel that completes no symbol writes no sample: its `out` may be NULL, as in tx_run)
        const bool writes = h && ((uint64_t)h->ncarry + nbits[c]) / h->bps > 0;
        scan = h && h->device == hs[0]->device && h->ph_kind == hs[0]->ph_kind &&
               (nbits[c] == 0 || (bits[c] && is_device_ptr(bits[c]))) &&
               (writes ? outs[c] && is_device_ptr(outs[c]) : !outs[c] || is_device_ptr(outs[c]));
        for (size_t e = 0; scan && e < c; ++e) scan = hs[e] != h;      // a handle at most once
    }
    if (scan) {
        for (size_t c = 0; c < nch; ++c) produced[c] = 0;
        return tx_scan_batch_run(hs, nch, bits, nbits, outs, caps, produced, s);
    }
    bool fuse = nch >= 2 && hs[0] != nullptr;
    for (size_t c = 0; fuse && c < nch; ++c) {
        const modem_tx* h = hs[c];
        const modem_tx* h0 = hs[0];
        fuse = h && h->device == h0->device && h->ph_kind == 0 && h->mfma_ksteps > 0 &&
               h->mfma_ksteps == h0->mfma_ksteps && h->out_mode == MODEM_OUT_IQ_MIXED && h->dtype == h0->dtype &&
               h->sps == h0->sps && h->bps == h0->bps && h->ntaps == h0->ntaps && h->q_offset == 0 &&
               h->bfrag_host == h0->bfrag_host && (nbits[c] == 0 || (bits[c] && is_device_ptr(bits[c]))) &&
               outs[c] && is_device_ptr(outs[c]);
        for (size_t e = 0; fuse && e < c; ++e) fuse = hs[e] != h;      // a handle at most once
    }
    if (!fuse) {
        for (size_t c = 0; c < nch; ++c) {
            const modem_status st = tx_run(hs[c], bits[c], nbits[c], false, outs[c], caps[c], &produced[c], s);
            if (st != MODEM_OK) return st;
        }
        return MODEM_OK;
    }
    for (size_t c = 0; c < nch; ++c) produced[c] = 0;
    // check every channel first: an error leaves all handles untouched
    std::vector<int64_t> nsym(nch);
    std::vector<int> ncarry_new(nch);
    for (size_t c = 0; c < nch; ++c) {
        const modem_tx* h = hs[c];
        const uint64_t total = (uint64_t)h->ncarry + nbits[c];
        nsym[c] = (int64_t)(total / h->bps);
        ncarry_new[c] = (int)(total - (uint64_t)nsym[c] * h->bps);
        if ((size_t)nsym[c] * h->sps > caps[c]) return MODEM_ERR_CAPACITY;
    }
    DeviceGuard g(hs[0]->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    for (size_t c0 = 0; c0 < nch; c0 += mk::kBatchMax) {
        mk::TxBatch b{};
        b.nch = (int32_t)std::min<size_t>(mk::kBatchMax, nch - c0);
        for (int i = 0; i < b.nch; ++i) {
            const size_t c = c0 + (size_t)i;
            tx_fill(hs[c], bits[c], nbits[c], false, outs[c], nsym[c], ncarry_new[c], (size_t)nsym[c] * hs[c]->sps, b.p[i]);
        }
        uint64_t launch_bytes = 0;          // the non-temporal split over the whole launch
        for (int i = 0; i < b.nch; ++i)
            launch_bytes += (uint64_t)nsym[c0 + i] * hs[c0 + i]->sps * tx_sample_bytes(hs[c0 + i]);
        for (int i = 0; i < b.nch; ++i)
            b.p[i].nt_below = tx_nt_below(nsym[c0 + i] * (int64_t)hs[c0 + i]->sps, launch_bytes, false);
        HIP_TRY(mk::launch_tx_mfma_batch(b, (int)hs[0]->sps, hs[0]->mfma_ksteps, hs[0]->d_bfrag, hs[0]->dtype, s));
        for (int i = 0; i < b.nch; ++i) {
            const size_t c = c0 + (size_t)i;
            modem_tx* h = hs[c];
            h->hcur ^= 1;
            h->ccur ^= 1;
            h->ncarry = ncarry_new[c];
            h->sample += (uint64_t)nsym[c] * h->sps;
            h->symbols += (uint64_t)nsym[c];
            produced[c] = (size_t)nsym[c] * h->sps;
        }
    }
    return MODEM_OK;
}
uint64_t modem_tx_sample(const modem_tx* h) { return h ? h->sample : 0; }
modem_status modem_tx_scan_states(const modem_tx* h, float* out, size_t cap, size_t* n, void* stream) {
    if (!h || !n) return MODEM_ERR_INVALID_ARG;
    *n = 0;
    if (!phasor_scanned(h->ph_kind)) return MODEM_ERR_UNSUPPORTED;
    *n = h->scan_n;
    if (cap < h->scan_n) return MODEM_ERR_CAPACITY;
    if (h->scan_n && !out) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    const hipStream_t s = (hipStream_t)stream;
    if (h->scan_n)
        HIP_TRY(hipMemcpyAsync(out, h->scan_stage.p, h->scan_n * sizeof(float2), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MODEM_OK;
}
int modem_tx_scan_path(const modem_tx* h) { return h ? h->scan_path : -1; }
modem_status modem_tx_destroy(modem_tx* h) { delete h; return MODEM_OK; }

// ------------------------------------------------------------------------------ RX ----
struct modem_rx {
    int device = 0;
    uint32_t ntaps = 0, decim = 1, D = 0, K = 1, HL = 0;
    int mix = 0, in_dtype = 0, out_dtype = 0;
    float w = 0.f;
    uint64_t c0 = 0;
    float phase_offset = 0.f;       // PLL offset (demodulator.rs:50)
    int64_t consumed = 0;          // stream samples processed
    modem_slicer_desc slicer{};
    int mfma_ksteps = 0;            // > 0: matched filter on the matrix pipe (rx_mfma)
    float* d_bfrag = nullptr;       // its split-f16 tap tables (modem_internal.h)
    std::vector<_Float16> bfrag_host;   // the same, on the host (batch compatibility check)
    int tap_scale_exp = 0;          // the tables hold h * 2^tap_scale_exp
    float* d_taps = nullptr;
    float2* d_slut = nullptr;
    void* d_hist[2] = {nullptr, nullptr};
    int* d_ka = nullptr;            // rx_mfma staging-exponent prediction, double-buffered like d_hist
    void* d_zeros = nullptr;
    int hcur = 0;
    Stage in_stage, iq_stage, sym_stage;
    ~modem_rx() {
        DeviceGuard g(device);
        for (void* p : {(void*)d_taps, (void*)d_slut, d_hist[0], d_hist[1], d_zeros, (void*)d_bfrag, (void*)d_ka})
            if (p) (void)hipFree(p);
    }
};

static size_t rx_in_bytes(const modem_rx* h) {
    return h->in_dtype == MODEM_DTYPE_I16 ? 2 : h->in_dtype == MODEM_DTYPE_F16 ? 4 : 8;
}
static size_t rx_out_bytes(const modem_rx* h) { return h->out_dtype == MODEM_DTYPE_F16 ? 4 : 8; }

modem_status modem_rx_create(const modem_rx_desc* d, int device, modem_rx** out) {
    if (!d || !out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (d->ntaps < 1 || d->ntaps > (uint32_t)mk::kMaxTaps || !d->taps) return MODEM_ERR_INVALID_ARG;
    if (d->decim < 1) return MODEM_ERR_INVALID_ARG;
    if (d->mix != MODEM_MIX_COMPLEX && d->mix != MODEM_MIX_REFERENCE_REAL && d->mix != MODEM_MIX_REFERENCE_REAL_EXACT)
        return MODEM_ERR_INVALID_ARG;
    if ((d->in_dtype != MODEM_DTYPE_F32 && d->in_dtype != MODEM_DTYPE_F16 && d->in_dtype != MODEM_DTYPE_I16) ||
        (d->out_dtype != MODEM_DTYPE_F32 && d->out_dtype != MODEM_DTYPE_F16)) return MODEM_ERR_INVALID_ARG;
    // real i16 input: the exact reference demodulator only (the complex kernels read I/Q pairs)
    if (d->in_dtype == MODEM_DTYPE_I16 && d->mix != MODEM_MIX_REFERENCE_REAL_EXACT) return MODEM_ERR_UNSUPPORTED;
    const modem_slicer_desc& sl = d->slicer;
    if (sl.kind == MODEM_SLICER_NEAREST && (sl.bits_per_symbol < 1 || sl.bits_per_symbol > 8 || !sl.lut))
        return MODEM_ERR_INVALID_ARG;
    if (sl.kind == MODEM_SLICER_QAM_AXIS && (sl.bits_per_carrier < 1 || sl.bits_per_carrier > 4))
        return MODEM_ERR_INVALID_ARG;
    if (sl.kind < MODEM_SLICER_NONE || sl.kind > MODEM_SLICER_QAM_AXIS) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_rx* h = new (std::nothrow) modem_rx;
    if (!h) return MODEM_ERR_ALLOC;
    h->device = device;
    h->ntaps = d->ntaps;
    h->decim = d->decim;
    h->D = d->decim_offset;
    h->K = (d->ntaps + d->decim - 1) / d->decim;
    h->HL = h->K * h->decim - 1;
    h->mix = d->mix;
    h->in_dtype = d->in_dtype;
    h->out_dtype = d->out_dtype;
    h->w = d->sample_freq;
    h->c0 = d->s0;
    h->phase_offset = d->phase_offset;
    h->slicer = sl;
    h->slicer.lut = nullptr;
    // pp[b*K + t] = h[b + decim*t], padded for the kernels' look-ahead tap loads
    std::vector<float> pp((size_t)h->K * h->decim + mk::kTapPad, 0.0f);
    for (uint32_t j = 0; j < d->ntaps; ++j) pp[(size_t)(j % h->decim) * h->K + j / h->decim] = d->taps[j];
    const size_t esz = rx_in_bytes(h);
    modem_status st;
    uint8_t *h0 = nullptr, *h1 = nullptr, *z = nullptr;
    if ((st = dalloc(&h->d_taps, pp.size())) || (st = dalloc(&h->d_slut, 256)) ||
        (st = dalloc(&h0, (h->HL + 1) * esz)) || (st = dalloc(&h1, (h->HL + 1) * esz)) ||
        (st = dalloc(&z, (size_t)(h->ntaps) * esz))) {
        h->d_hist[0] = h0; h->d_hist[1] = h1; h->d_zeros = z;
        delete h;
        return st;
    }
    h->d_hist[0] = h0; h->d_hist[1] = h1; h->d_zeros = z;
    const int ka_none[2] = {INT32_MIN, INT32_MIN};
    if ((st = dalloc(&h->d_ka, 2))) { delete h; return st; }
    if (hipMemcpy(h->d_taps, pp.data(), pp.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_ka, ka_none, sizeof ka_none, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); delete h; return MODEM_ERR_HIP;
    }
    if (sl.kind == MODEM_SLICER_NEAREST &&
        hipMemcpy(h->d_slut, sl.lut, ((size_t)2 << sl.bits_per_symbol) * sizeof(float),
                  hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); delete h; return MODEM_ERR_HIP;
    }
    const char* env = std::getenv("MODEM_HIP_FIR");
    const bool force_valu = env && std::strcmp(env, "valu") == 0;
    const bool exact = h->mix == MODEM_MIX_REFERENCE_REAL_EXACT;
    h->mfma_ksteps = force_valu || exact ? 0 : mk::rx_mfma_ksteps((int)h->decim, (int)h->ntaps);
    if (h->mfma_ksteps > 0) {
        // Split-f16 tap tables of rx_mfma (modem_rx.hip): the reversed taps T[x] = h[W-1-x]
        // scaled by 2^kb (exact; 0 when max |h| is in [2^-3, 2^15), else into [2^14, 2^15)), as f16
        // hi then lo = rn_f16(v - hi), in NC copies shifted by gcd(decim, 8) so that every
        // lane's 8-tap read is 16-B aligned.
        const int nks = h->mfma_ksteps, W = 32 * nks, dec = (int)h->decim;
        const int nc = mk::rx_mfma_table_copies(dec), tb = mk::rx_mfma_table_len(dec, nks), gq = 8 / nc;
        float hmax = 0.0f;
        for (uint32_t k = 0; k < h->ntaps; ++k) hmax = std::max(hmax, std::fabs(d->taps[k]));
        int kb = 0;   // 0 inside [2^-3, 2^15), else into [2^14, 2^15)
        if (hmax > 0.0f && std::isfinite(hmax) && !(hmax >= 0.125f && hmax < 32768.0f)) {
            int e;
            std::frexp(hmax, &e);
            kb = 15 - e;
        }
        h->tap_scale_exp = kb;
        std::vector<_Float16> tab((size_t)nc * 2 * tb, (_Float16)0.0f);
        for (int c = 0; c < nc; ++c)
            for (int y = 0; y < tb; ++y) {
                const int u = W - 1 - (y + c * gq);
                const float v = (u >= 0 && u < (int)h->ntaps) ? std::ldexp(d->taps[u], kb) : 0.0f;
                const _Float16 hi = (_Float16)v;
                tab[((size_t)c * 2) * tb + y] = hi;
                tab[((size_t)c * 2 + 1) * tb + y] = (_Float16)(v - (float)hi);
            }
        const size_t nfl = (tab.size() * sizeof(_Float16) + sizeof(float) - 1) / sizeof(float);
        if ((st = dalloc(&h->d_bfrag, nfl))) { delete h; return st; }
        h->bfrag_host = tab;
        if (hipMemcpy(h->d_bfrag, tab.data(), tab.size() * sizeof(_Float16), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError(); delete h; return MODEM_ERR_HIP;
        }
    }
    *out = h;
    return MODEM_OK;
}

// Kept instants n = k*decim + D with n in [a, b): first k and count.
static void rx_range(int64_t a, int64_t b, int64_t decim, int64_t D, int64_t* k0, int64_t* cnt) {
    auto first_at_or_after = [&](int64_t n) -> int64_t {
        return n <= D ? 0 : (n - D + decim - 1) / decim;
    };
    *k0 = first_at_or_after(a);
    const int64_t k1 = first_at_or_after(b);
    *cnt = k1 > *k0 ? k1 - *k0 : 0;
}

// Kernel parameters of one RX call on device buffers; see rx_run.
static void rx_fill(const modem_rx* h, const void* din, size_t n, void* diq, uint8_t* dsym, int64_t k_first,
                    int64_t nout, mk::RxParams& p) {
    p.x = din;
    p.hist = h->d_hist[h->hcur];
    p.hist_new = h->d_hist[h->hcur ^ 1];
    p.out_iq = nout ? diq : nullptr;
    p.out_sym = nout ? dsym : nullptr;
    p.taps = h->d_taps;
    p.slut = h->d_slut;
    p.N = (int64_t)n;
    p.n_start = h->consumed;
    p.c0 = h->c0;
    p.k_first = k_first;
    p.nout = nout;
    p.K = (int)h->K;
    p.L = (int)h->ntaps;
    p.HL = (int)h->HL;
    p.D = (int)h->D;
    p.decim = (int)h->decim;
    p.x_aligned16 = ((uintptr_t)din % 16) == 0 ? 1 : 0;
    p.phase_offset = h->phase_offset;
    p.exact_idx = (h->c0 + (uint64_t)h->consumed + n + (uint64_t)h->HL) <= (1ull << 53) ? 1 : 0;
    p.idx46 = (h->c0 + (uint64_t)h->consumed + n + (uint64_t)h->HL + 65536) < (1ull << 46) ? 1 : 0;
    p.ka_in = h->d_ka + h->hcur;
    p.ka_out = h->d_ka + (h->hcur ^ 1);
    p.slicer_kind = h->slicer.kind;
    p.bps = (int)h->slicer.bits_per_symbol;
    p.bits_per_carrier = (int)h->slicer.bits_per_carrier;
    p.inv_scale = h->slicer.inv_scale;
    p.max_symbol = h->slicer.max_symbol;
    p.w = h->w;
    p.tap_scale_exp = h->tap_scale_exp;
}

// The handle's state after an RX call (the kernel wrote the other history / ka slot).
static void rx_advance(modem_rx* h, size_t n) {
    h->hcur ^= 1;
    h->consumed += (int64_t)n;
}

// The kernel launch of one RX call on device buffers and the handle's state update.
static modem_status rx_launch(modem_rx* h, const void* din, size_t n, void* diq, uint8_t* dsym, int64_t k_first,
                              int64_t nout, hipStream_t s) {
    mk::RxParams p{};
    rx_fill(h, din, n, diq, dsym, k_first, nout, p);
    if (h->mfma_ksteps > 0) {
        HIP_TRY(mk::launch_rx_mfma(p, (int)h->decim, h->mfma_ksteps, h->d_bfrag, h->in_dtype, h->out_dtype,
                                   h->mix, s));
    } else
        HIP_TRY(mk::launch_rx(p, (int)h->decim, h->in_dtype, h->out_dtype, h->mix, s));
    rx_advance(h, n);
    return MODEM_OK;
}

static modem_status rx_run(modem_rx* h, const void* in, size_t n, bool zeros, void* out_iq,
                           uint8_t* out_sym, size_t cap, size_t* produced, hipStream_t s) {
    if (!h || !produced || (n && !in && !zeros)) return MODEM_ERR_INVALID_ARG;
    *produced = 0;
    int64_t k_first, nout;
    rx_range(h->consumed, h->consumed + (int64_t)n, h->decim, h->D, &k_first, &nout);
    if ((size_t)nout > cap) return MODEM_ERR_CAPACITY;
    const PtrKind ki = n && !zeros ? ptr_kind(in, h->device) : PTR_DEVICE;
    const PtrKind kq = nout && out_iq ? ptr_kind(out_iq, h->device) : PTR_DEVICE;
    const PtrKind ks = nout && out_sym ? ptr_kind(out_sym, h->device) : PTR_DEVICE;
    if (ki == PTR_FOREIGN || kq == PTR_FOREIGN || ks == PTR_FOREIGN) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    const void* din = zeros ? h->d_zeros : in;
    if (ki == PTR_HOST) {
        if ((st = h->in_stage.ensure(n * rx_in_bytes(h)))) return st;
        HIP_TRY(hipMemcpyAsync(h->in_stage.p, in, n * rx_in_bytes(h), hipMemcpyHostToDevice, s));
        din = h->in_stage.p;
    }
    const bool host_iq = kq == PTR_HOST;
    const bool host_sym = ks == PTR_HOST;
    void* diq = out_iq;
    uint8_t* dsym = out_sym;
    if (host_iq) {
        if ((st = h->iq_stage.ensure((size_t)nout * rx_out_bytes(h)))) return st;
        diq = h->iq_stage.p;
    }
    if (host_sym) {
        if ((st = h->sym_stage.ensure((size_t)nout))) return st;
        dsym = static_cast<uint8_t*>(h->sym_stage.p);
    }
    if ((st = rx_launch(h, din, n, diq, dsym, k_first, nout, s))) return st;
    if (host_iq) HIP_TRY(hipMemcpyAsync(out_iq, diq, (size_t)nout * rx_out_bytes(h), hipMemcpyDeviceToHost, s));
    if (host_sym) HIP_TRY(hipMemcpyAsync(out_sym, dsym, (size_t)nout, hipMemcpyDeviceToHost, s));
    if (host_iq || host_sym || din == h->in_stage.p) HIP_TRY(hipStreamSynchronize(s));
    *produced = (size_t)nout;
    return MODEM_OK;
}

modem_status modem_rx_process(modem_rx* h, const void* in, size_t n, void* out_iq, uint8_t* out_sym,
                              size_t cap, size_t* produced, void* stream) {
    return rx_run(h, in, n, false, out_iq, out_sym, cap, produced, (hipStream_t)stream);
}
modem_status modem_rx_flush(modem_rx* h, void* out_iq, uint8_t* out_sym, size_t cap, size_t* produced,
                            void* stream) {
    if (!h) return MODEM_ERR_INVALID_ARG;
    return rx_run(h, nullptr, h->ntaps - 1, true, out_iq, out_sym, cap, produced, (hipStream_t)stream);
}
// One launch for several channels; equivalent to modem_rx_process on each in order. Fused
// per kBatchMax channels when every handle shares the matrix-core configuration (decim,
// taps, complex mix, one I/Q dtype in and out, device) and all buffers are device memory.
modem_status modem_rx_process_batch(modem_rx* const* hs, size_t nch, const void* const* ins, const size_t* ns,
                                    void* const* out_iq, uint8_t* const* out_sym, const size_t* caps,
                                    size_t* produced, void* stream) {
    if (nch == 0) return MODEM_OK;
    if (!hs || !ins || !ns || !out_iq || !out_sym || !caps || !produced) return MODEM_ERR_INVALID_ARG;
    const hipStream_t s = (hipStream_t)stream;
    for (size_t c = 0; c < nch; ++c)
        if (hs[c] && ((ns[c] && foreign_ptr(ins[c], hs[c]->device)) || foreign_ptr(out_iq[c], hs[c]->device) ||
                      foreign_ptr(out_sym[c], hs[c]->device)))
            return MODEM_ERR_INVALID_ARG;
    bool fuse = nch >= 2 && hs[0] != nullptr;
    for (size_t c = 0; fuse && c < nch; ++c) {
        const modem_rx* h = hs[c];
        const modem_rx* h0 = hs[0];
        fuse = h && h->device == h0->device && h->mfma_ksteps > 0 && h->mfma_ksteps == h0->mfma_ksteps &&
               h->mix == MODEM_MIX_COMPLEX && h->in_dtype == h0->in_dtype && h->out_dtype == h->in_dtype &&
               h->decim == h0->decim && h->ntaps == h0->ntaps && h->bfrag_host == h0->bfrag_host &&
               (ns[c] == 0 || (ins[c] && is_device_ptr(ins[c]))) &&
               (!out_iq[c] || is_device_ptr(out_iq[c])) && (!out_sym[c] || is_device_ptr(out_sym[c]));
        for (size_t e = 0; fuse && e < c; ++e) fuse = hs[e] != h;
    }
    if (!fuse) {
        for (size_t c = 0; c < nch; ++c) {
            const modem_status st = rx_run(hs[c], ins[c], ns[c], false, out_iq[c], out_sym[c], caps[c],
                                           &produced[c], s);
            if (st != MODEM_OK) return st;
        }
        return MODEM_OK;
    }
    for (size_t c = 0; c < nch; ++c) produced[c] = 0;
    std::vector<int64_t> k_first(nch), nout(nch);
    for (size_t c = 0; c < nch; ++c) {
        const modem_rx* h = hs[c];
        rx_range(h->consumed, h->consumed + (int64_t)ns[c], h->decim, h->D, &k_first[c], &nout[c]);
        if ((size_t)nout[c] > caps[c]) return MODEM_ERR_CAPACITY;
    }
    DeviceGuard g(hs[0]->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    for (size_t c0 = 0; c0 < nch; c0 += mk::kBatchMax) {
        mk::RxBatch b{};
        b.nch = (int32_t)std::min<size_t>(mk::kBatchMax, nch - c0);
        for (int i = 0; i < b.nch; ++i) {
            const size_t c = c0 + (size_t)i;
            rx_fill(hs[c], ins[c], ns[c], out_iq[c], out_sym[c], k_first[c], nout[c], b.p[i]);
        }
        HIP_TRY(mk::launch_rx_mfma_batch(b, (int)hs[0]->decim, hs[0]->mfma_ksteps, hs[0]->d_bfrag,
                                         hs[0]->in_dtype, s));
        for (int i = 0; i < b.nch; ++i) {
            const size_t c = c0 + (size_t)i;
            hs[c]->hcur ^= 1;
            hs[c]->consumed += (int64_t)ns[c];
            produced[c] = (size_t)nout[c];
        }
    }
    return MODEM_OK;
}
uint64_t modem_rx_sample(const modem_rx* h) { return h ? h->c0 + (uint64_t)h->consumed : 0; }
modem_status modem_rx_destroy(modem_rx* h) { delete h; return MODEM_OK; }

// ---------------------------------------------------------------------------- chain ----
// A prepared TX -> RX step over fixed device buffers: the buffers' kinds are checked once here,
// so a step is one launch (modem_chain.hip: TX and RX of the period fused, where the filters
// and the call's geometry allow; MODEM_CHAIN_FUSED=0 in the environment at create time turns
// it off) or the two launches, and the state updates (tx_run / rx_run minus the pointer
// queries and staging decisions, ~1 us of host time each per call).
struct modem_chain {
    bool fused = true;
    int last = -1;             // how the last run ran (modem_chain_fused)
    bool verbose = false;      // MODEM_CHAIN_VERBOSE=1: why a run took the two launches (stderr)
    modem_tx* tx = nullptr;
    modem_rx* rx = nullptr;
    const uint8_t* bits = nullptr;
    size_t nbits = 0;
    void* samples = nullptr;
    size_t cap = 0;
    void* out_iq = nullptr;
    uint8_t* out_sym = nullptr;
    size_t out_cap = 0;
};

modem_status modem_chain_create(modem_tx* tx, modem_rx* rx, const uint8_t* bits, size_t nbits, void* samples,
                                size_t cap, void* out_iq, uint8_t* out_sym, size_t out_cap, modem_chain** out) {
    if (!tx || !rx || !out || !samples || (nbits && !bits)) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (tx->device != rx->device) return MODEM_ERR_INVALID_ARG;
    // the RX reads what the TX writes: interleaved complex samples of one dtype
    if (tx->out_mode == MODEM_OUT_REAL || rx->in_dtype != tx->dtype) return MODEM_ERR_INVALID_ARG;
    const int dev = tx->device;
    if ((nbits && ptr_kind(bits, dev) != PTR_DEVICE) || ptr_kind(samples, dev) != PTR_DEVICE ||
        (out_iq && ptr_kind(out_iq, dev) != PTR_DEVICE) || (out_sym && ptr_kind(out_sym, dev) != PTR_DEVICE))
        return MODEM_ERR_INVALID_ARG;
    modem_chain* c = new (std::nothrow) modem_chain;
    if (!c) return MODEM_ERR_ALLOC;
    c->tx = tx; c->rx = rx; c->bits = bits; c->nbits = nbits; c->samples = samples; c->cap = cap;
    c->out_iq = out_iq; c->out_sym = out_sym; c->out_cap = out_cap;
    const char* env = std::getenv("MODEM_CHAIN_FUSED");
    c->fused = !(env && env[0] == '0');
    const char* verb = std::getenv("MODEM_CHAIN_VERBOSE");
    c->verbose = verb && verb[0] == '1';
    *out = c;
    return MODEM_OK;
}

modem_status modem_chain_run(modem_chain* c, size_t* produced, size_t* produced_out, void* stream) {
    if (!c || !produced || !produced_out) return MODEM_ERR_INVALID_ARG;
    *produced = *produced_out = 0;
    modem_tx* tx = c->tx;
    modem_rx* rx = c->rx;
    const hipStream_t s = (hipStream_t)stream;
    const uint64_t total = (uint64_t)tx->ncarry + c->nbits;
    const int64_t nsym = (int64_t)(total / tx->bps);
    const int ncarry_new = (int)(total - (uint64_t)nsym * tx->bps);
    const size_t nsamp = (size_t)nsym * tx->sps;
    if (nsamp > c->cap) return MODEM_ERR_CAPACITY;
    int64_t k_first, nout;
    rx_range(rx->consumed, rx->consumed + (int64_t)nsamp, rx->decim, rx->D, &k_first, &nout);
    if ((size_t)nout > c->out_cap) return MODEM_ERR_CAPACITY;
    DeviceGuard g(tx->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    const bool eligible = c->fused && !tx->ph_kind && tx->mfma_ksteps > 0 && rx->mfma_ksteps > 0 &&
                          rx->mix == MODEM_MIX_COMPLEX && tx->out_mode == MODEM_OUT_IQ_MIXED &&
                          rx->out_dtype == rx->in_dtype && tx->sps == rx->decim && nout > 0;
    if (c->verbose && !eligible)
        std::fprintf(stderr, "modem_chain_run: two launches (fused %d ph %d tx ks %d rx ks %d mix %d out_mode %d "
                     "dtypes %d/%d sps %u decim %u nout %lld)\n", (int)c->fused, (int)tx->ph_kind, tx->mfma_ksteps,
                     rx->mfma_ksteps, (int)rx->mix, (int)tx->out_mode, (int)rx->in_dtype, (int)rx->out_dtype,
                     (unsigned)tx->sps, (unsigned)rx->decim, (long long)nout);
    if (eligible) {
        mk::TxParams tp{};
        tx_fill(tx, c->bits, c->nbits, false, c->samples, nsym, ncarry_new, nsamp, tp);
        mk::RxParams rp{};
        rx_fill(rx, c->samples, nsamp, c->out_iq, c->out_sym, k_first, nout, rp);
        int form = 1;
        const hipError_t e = mk::launch_chain_mfma(tp, (int)tx->sps, tx->mfma_ksteps, tx->d_bfrag, rp, rx->mfma_ksteps,
                                                   rx->d_bfrag, tx->dtype, s, &form);
        if (e == hipSuccess) {
            c->last = form;
            tx_advance(tx, false, nsym, ncarry_new, nsamp);
            rx_advance(rx, nsamp);
            *produced = nsamp;
            *produced_out = (size_t)nout;
            return MODEM_OK;
        }
        if (e != hipErrorNotSupported) { (void)hipGetLastError(); return MODEM_ERR_HIP; }
        if (c->verbose) std::fprintf(stderr, "modem_chain_run: no fused form for this call (two launches)\n");
    }
    if ((st = tx_launch(tx, c->bits, c->nbits, false, c->samples, nsym, ncarry_new, nsamp, s))) return st;
    if ((st = rx_launch(rx, c->samples, nsamp, nout ? c->out_iq : nullptr, nout ? c->out_sym : nullptr, k_first,
                        nout, s)))
        return st;
    c->last = 0;
    *produced = nsamp;
    *produced_out = (size_t)nout;
    return MODEM_OK;
}

int modem_chain_fused(const modem_chain* c) { return c ? c->last : -1; }

modem_status modem_chain_destroy(modem_chain* c) { delete c; return MODEM_OK; }

// ----------------------------------------------------------------------- chain batch ----
// A prepared period of a channel bank over fixed device buffers (BASELINE config 4): the
// handles' batch compatibility and the buffers' kinds are checked once here (modem_tx_process_batch
// and modem_rx_process_batch check them on every call: a pointer-attribute query per buffer and a
// comparison of the handles' fragment tables, ~10 us per 4-channel TX call, which held C4's
// channel groups to the host's rate), so a run is the launches and the state updates.
struct modem_chain_batch {
    std::vector<modem_tx*> tx;
    std::vector<modem_rx*> rx;
    std::vector<const uint8_t*> bits;
    std::vector<size_t> nbits, caps, out_caps;
    std::vector<void*> samples, out_iq;
    std::vector<uint8_t*> out_sym;
    size_t group = mk::kBatchMax;
    // Two lanes: group k's TX and RX launches go to the caller's stream (k even) or to the plan's
    // own stream (k odd), joined to the caller's stream by events at the start and the end of a
    // run, so that a group's RX runs beside the next group's TX (each launch's tail of straggling
    // workgroups is filled by the other lane's head). A group stays on its lane from run to run,
    // so each handle's calls keep their order. C4's 64-channel job: 1.049 -> 0.950 ms per step
    // in groups of 8, 1.090 -> 0.948 in groups of 4 (profiles/r05_c4_job.txt).
    // MODEM_CHAIN_BATCH_LANES=1 in the environment at create time: one lane.
    hipStream_t side = nullptr;
    hipEvent_t ev_start = nullptr, ev_end = nullptr;
    bool failed = false;                // a launch of a run failed (modem_chain_batch_run)
    ~modem_chain_batch() {
        if (ev_start) (void)hipEventDestroy(ev_start);
        if (ev_end) (void)hipEventDestroy(ev_end);
        if (side) (void)hipStreamDestroy(side);
    }
};

modem_status modem_chain_batch_create(modem_tx* const* txs, modem_rx* const* rxs, size_t nch, size_t group,
                                      const uint8_t* const* bits, const size_t* nbits, void* const* samples,
                                      const size_t* caps, void* const* out_iq, uint8_t* const* out_sym,
                                      const size_t* out_caps, modem_chain_batch** out) {
    if (!out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (!txs || !rxs || nch == 0 || group < 1 || group > (size_t)mk::kBatchMax || !bits || !nbits || !samples ||
        !caps || !out_iq || !out_sym || !out_caps)
        return MODEM_ERR_INVALID_ARG;
    const modem_tx* t0 = txs[0];
    const modem_rx* r0 = rxs[0];
    if (!t0 || !r0) return MODEM_ERR_INVALID_ARG;
    const int dev = t0->device;
    for (size_t c = 0; c < nch; ++c) {
        const modem_tx* t = txs[c];
        const modem_rx* r = rxs[c];
        if (!t || !r || t->device != dev || r->device != dev || !samples[c] || (nbits[c] && !bits[c]))
            return MODEM_ERR_INVALID_ARG;
        for (size_t e = 0; e < c; ++e)
            if (txs[e] == t || rxs[e] == r) return MODEM_ERR_INVALID_ARG;   // a handle at most once
        // the RX reads what the TX writes: interleaved complex samples of one dtype
        if (t->out_mode != MODEM_OUT_IQ_MIXED || r->in_dtype != t->dtype) return MODEM_ERR_INVALID_ARG;
        if ((nbits[c] && ptr_kind(bits[c], dev) != PTR_DEVICE) || ptr_kind(samples[c], dev) != PTR_DEVICE ||
            (out_iq[c] && ptr_kind(out_iq[c], dev) != PTR_DEVICE) ||
            (out_sym[c] && ptr_kind(out_sym[c], dev) != PTR_DEVICE))
            return MODEM_ERR_INVALID_ARG;
        // one matrix-core configuration per side (the batch kernels' conditions)
        if (t->ph_kind != 0 || t->mfma_ksteps <= 0 || t->mfma_ksteps != t0->mfma_ksteps || t->dtype != t0->dtype ||
            t->sps != t0->sps || t->bps != t0->bps || t->ntaps != t0->ntaps || t->q_offset != 0 ||
            t->bfrag_host != t0->bfrag_host)
            return MODEM_ERR_UNSUPPORTED;
        if (r->mfma_ksteps <= 0 || r->mfma_ksteps != r0->mfma_ksteps || r->mix != MODEM_MIX_COMPLEX ||
            r->in_dtype != r0->in_dtype || r->out_dtype != r->in_dtype || r->decim != r0->decim ||
            r->ntaps != r0->ntaps || r->bfrag_host != r0->bfrag_host)
            return MODEM_ERR_UNSUPPORTED;
    }
    modem_chain_batch* b = new (std::nothrow) modem_chain_batch;
    if (!b) return MODEM_ERR_ALLOC;
    const char* lanes = std::getenv("MODEM_CHAIN_BATCH_LANES");
    if (nch > group && !(lanes && lanes[0] == '1')) {
        DeviceGuard g(dev);
        if (!g.ok) { delete b; return MODEM_ERR_NO_DEVICE; }
        if (hipStreamCreateWithFlags(&b->side, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&b->ev_start, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&b->ev_end, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            delete b;
            return MODEM_ERR_HIP;
        }
    }
    b->tx.assign(txs, txs + nch);
    b->rx.assign(rxs, rxs + nch);
    b->bits.assign(bits, bits + nch);
    b->nbits.assign(nbits, nbits + nch);
    b->samples.assign(samples, samples + nch);
    b->caps.assign(caps, caps + nch);
    b->out_iq.assign(out_iq, out_iq + nch);
    b->out_sym.assign(out_sym, out_sym + nch);
    b->out_caps.assign(out_caps, out_caps + nch);
    b->group = group;
    *out = b;
    return MODEM_OK;
}

// The launches of one run, group by group (after the checks of modem_chain_batch_run).
static modem_status chain_batch_launch(modem_chain_batch* b, hipStream_t s, size_t* produced, size_t* produced_out) {
    const size_t nch = b->tx.size();
    int64_t nsym[mk::kBatchMax], k_first[mk::kBatchMax], nout[mk::kBatchMax];
    int ncarry_new[mk::kBatchMax];
    for (size_t c0 = 0; c0 < nch; c0 += b->group) {
        const int n = (int)std::min(b->group, nch - c0);
        const hipStream_t ls = b->side && (c0 / b->group) % 2 ? b->side : s;   // this group's lane
        mk::TxBatch tb{};
        tb.nch = n;
        uint64_t launch_bytes = 0;
        for (int i = 0; i < n; ++i) {
            const size_t c = c0 + (size_t)i;
            const modem_tx* t = b->tx[c];
            const uint64_t total = (uint64_t)t->ncarry + b->nbits[c];
            nsym[i] = (int64_t)(total / t->bps);
            ncarry_new[i] = (int)(total - (uint64_t)nsym[i] * t->bps);
            const size_t ns = (size_t)nsym[i] * t->sps;
            tx_fill(t, b->bits[c], b->nbits[c], false, b->samples[c], nsym[i], ncarry_new[i], ns, tb.p[i]);
            launch_bytes += (uint64_t)ns * tx_sample_bytes(t);
        }
        for (int i = 0; i < n; ++i)
            tb.p[i].nt_below = tx_nt_below(nsym[i] * (int64_t)b->tx[c0 + i]->sps, launch_bytes, false);
        const modem_tx* t0 = b->tx[c0];
        HIP_TRY(mk::launch_tx_mfma_batch(tb, (int)t0->sps, t0->mfma_ksteps, t0->d_bfrag, t0->dtype, ls));
        mk::RxBatch rb{};
        rb.nch = n;
        for (int i = 0; i < n; ++i) {
            const size_t c = c0 + (size_t)i;
            modem_tx* t = b->tx[c];
            const size_t ns = (size_t)nsym[i] * t->sps;
            tx_advance(t, false, nsym[i], ncarry_new[i], ns);
            modem_rx* r = b->rx[c];
            rx_range(r->consumed, r->consumed + (int64_t)ns, r->decim, r->D, &k_first[i], &nout[i]);
            rx_fill(r, b->samples[c], ns, b->out_iq[c], b->out_sym[c], k_first[i], nout[i], rb.p[i]);
            if (produced) produced[c] = ns;
            if (produced_out) produced_out[c] = (size_t)nout[i];
        }
        const modem_rx* r0 = b->rx[c0];
        HIP_TRY(mk::launch_rx_mfma_batch(rb, (int)r0->decim, r0->mfma_ksteps, r0->d_bfrag, r0->in_dtype, ls));
        for (int i = 0; i < n; ++i) rx_advance(b->rx[c0 + i], (size_t)nsym[i] * b->tx[c0 + i]->sps);
    }
    return MODEM_OK;
}

modem_status modem_chain_batch_run(modem_chain_batch* b, size_t* produced, size_t* produced_out, void* stream) {
    if (!b) return MODEM_ERR_INVALID_ARG;
    // a launch failed in an earlier run: some groups' handles advanced and others not, so the
    // channels' streams no longer line up (the plan and its handles are unusable)
    if (b->failed) return MODEM_ERR_HIP;
    const size_t nch = b->tx.size();
    const hipStream_t s = (hipStream_t)stream;
    // every channel's call sizes first: an error here leaves every handle untouched
    for (size_t c = 0; c < nch; ++c) {
        const modem_tx* t = b->tx[c];
        const uint64_t total = (uint64_t)t->ncarry + b->nbits[c];
        const int64_t ns = (int64_t)(total / t->bps);
        if ((size_t)ns * t->sps > b->caps[c]) return MODEM_ERR_CAPACITY;
        int64_t k0, k;
        rx_range(b->rx[c]->consumed, b->rx[c]->consumed + ns * (int64_t)t->sps, b->rx[c]->decim, b->rx[c]->D, &k0, &k);
        if ((size_t)k > b->out_caps[c]) return MODEM_ERR_CAPACITY;
    }
    DeviceGuard g(b->tx[0]->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    if (b->side) {                              // the plan's lane starts after what precedes the run
        HIP_TRY(hipEventRecord(b->ev_start, s));
        HIP_TRY(hipStreamWaitEvent(b->side, b->ev_start, 0));
    }
    const modem_status st = chain_batch_launch(b, s, produced, produced_out);
    if (b->side) {                              // the caller's stream continues after both lanes:
        // also after a failed launch (best effort), so that the caller's stream is still ordered
        // after the side lane's kernels already queued
        const bool joined = hipEventRecord(b->ev_end, b->side) == hipSuccess &&
                            hipStreamWaitEvent(s, b->ev_end, 0) == hipSuccess;
        if (st == MODEM_OK && !joined) { (void)hipGetLastError(); b->failed = true; return MODEM_ERR_HIP; }
    }
    if (st != MODEM_OK) b->failed = true;
    return st;
}

modem_status modem_chain_batch_destroy(modem_chain_batch* b) { delete b; return MODEM_OK; }

// ----------------------------------------------------------------------------- FIR ----
struct modem_fir {
    int device = 0;
    uint32_t L = 0;
    float* d_taps = nullptr;
    float* d_hist[2] = {nullptr, nullptr};
    int hcur = 0;
    Stage in_stage, out_stage;
    ~modem_fir() {
        DeviceGuard g(device);
        for (void* p : {(void*)d_taps, (void*)d_hist[0], (void*)d_hist[1]}) if (p) (void)hipFree(p);
    }
};

modem_status modem_fir_create(const float* taps, uint32_t ntaps, int device, modem_fir** out) {
    // FIRFilter::new(&[]) would divide by zero in add() (fir.rs:31): reject it here.
    if (!out || !taps || ntaps < 1 || ntaps > (uint32_t)mk::kMaxTaps) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_fir* h = new (std::nothrow) modem_fir;
    if (!h) return MODEM_ERR_ALLOC;
    h->device = device;
    h->L = ntaps;
    modem_status st;
    if ((st = dalloc(&h->d_taps, ntaps)) || (st = dalloc(&h->d_hist[0], ntaps)) ||
        (st = dalloc(&h->d_hist[1], ntaps))) { delete h; return st; }
    if (hipMemcpy(h->d_taps, taps, ntaps * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); delete h; return MODEM_ERR_HIP;
    }
    *out = h;
    return MODEM_OK;
}

modem_status modem_fir_process(modem_fir* h, const float* in, float* out, size_t n, void* stream) {
    if (!h || (n && (!in || !out))) return MODEM_ERR_INVALID_ARG;
    const PtrKind ki = n ? ptr_kind(in, h->device) : PTR_DEVICE, ko = n ? ptr_kind(out, h->device) : PTR_DEVICE;
    if (ki == PTR_FOREIGN || ko == PTR_FOREIGN) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    modem_status st;
    const float* din = in;
    float* dout = out;
    if (ki == PTR_HOST) {
        if ((st = h->in_stage.ensure(n * sizeof(float)))) return st;
        HIP_TRY(hipMemcpyAsync(h->in_stage.p, in, n * sizeof(float), hipMemcpyHostToDevice, s));
        din = static_cast<const float*>(h->in_stage.p);
    }
    const bool host_out = ko == PTR_HOST;
    if (host_out) {
        if ((st = h->out_stage.ensure(n * sizeof(float)))) return st;
        dout = static_cast<float*>(h->out_stage.p);
    }
    mk::FirParams p{};
    p.x = din;
    p.hist = h->d_hist[h->hcur];
    p.hist_new = h->d_hist[h->hcur ^ 1];
    p.y = dout;
    p.taps = h->d_taps;
    p.N = (int64_t)n;
    p.L = (int)h->L;
    HIP_TRY(mk::launch_fir(p, s));
    h->hcur ^= 1;
    if (host_out) HIP_TRY(hipMemcpyAsync(out, dout, n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (host_out || din != in) HIP_TRY(hipStreamSynchronize(s));
    return MODEM_OK;
}

modem_status modem_fir_destroy(modem_fir* h) { delete h; return MODEM_OK; }

// ------------------------------------------------------------------- soft demapper ----
struct modem_demap {
    int device = 0;
    uint32_t bps = 0;
    int32_t in_dtype = 0, out_dtype = 0;
    bool axis = false;
    float* d_tab = nullptr;   // general: the 2^bps (i, q) points; axis: the I levels, then the Q levels
    Stage in_stage, out_stage;
    ~modem_demap() {
        DeviceGuard g(device);
        if (d_tab) (void)hipFree(d_tab);
    }
};

// The table is a product grid with an even bit split, bitwise: lut[2((a<<h)|b)] depends only on
// a, lut[2((a<<h)|b)+1] only on b (h = bps/2). levels: its 2^h I values, then its 2^h Q values —
// the table's own floats, so the axis path's inputs are the general path's.
static bool demap_axis_levels(const float* lut, uint32_t bps, std::vector<float>* levels) {
    if (bps % 2) return false;
    const uint32_t h = bps / 2, n = 1u << h;
    levels->resize(2 * n);
    for (uint32_t a = 0; a < n; ++a) {
        (*levels)[a] = lut[2 * (a << h)];
        (*levels)[n + a] = lut[2 * a + 1];
    }
    for (uint32_t a = 0; a < n; ++a)
        for (uint32_t b = 0; b < n; ++b) {
            const float* pt = lut + 2 * ((a << h) | b);
            if (std::memcmp(&pt[0], &(*levels)[a], sizeof(float)) != 0 ||
                std::memcmp(&pt[1], &(*levels)[n + b], sizeof(float)) != 0) return false;
        }
    return true;
}

static size_t demap_out_bytes(int32_t dt) { return dt == MODEM_DTYPE_F32 ? 4 : dt == MODEM_DTYPE_F16 ? 2 : 1; }

modem_status modem_demap_create(const float* lut, uint32_t bits_per_symbol, int32_t in_dtype, int32_t out_dtype,
                                int32_t path, int device, modem_demap** out) {
    if (!out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (!lut || bits_per_symbol < 1 || bits_per_symbol > 8) return MODEM_ERR_INVALID_ARG;
    if (in_dtype != MODEM_DTYPE_F32 && in_dtype != MODEM_DTYPE_F16) return MODEM_ERR_INVALID_ARG;
    if (out_dtype != MODEM_DTYPE_F32 && out_dtype != MODEM_DTYPE_F16 && out_dtype != MODEM_DTYPE_I8)
        return MODEM_ERR_INVALID_ARG;
    if (path != MODEM_DEMAP_AUTO && path != MODEM_DEMAP_GENERAL) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_demap* h = new (std::nothrow) modem_demap;
    if (!h) return MODEM_ERR_ALLOC;
    h->device = device;
    h->bps = bits_per_symbol;
    h->in_dtype = in_dtype;
    h->out_dtype = out_dtype;
    std::vector<float> levels;
    h->axis = path == MODEM_DEMAP_AUTO && demap_axis_levels(lut, bits_per_symbol, &levels);
    const float* tab = h->axis ? levels.data() : lut;
    const size_t ntab = h->axis ? levels.size() : (size_t)2 << bits_per_symbol;
    modem_status st;
    if ((st = dalloc(&h->d_tab, ntab))) { delete h; return st; }
    if (hipMemcpy(h->d_tab, tab, ntab * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); delete h; return MODEM_ERR_HIP;
    }
    *out = h;
    return MODEM_OK;
}

modem_status modem_demap_process(modem_demap* h, const void* iq, size_t nsym, float scale, void* llr, size_t cap,
                                 void* stream) {
    if (!h || !std::isfinite(scale) || (nsym && (!iq || !llr))) return MODEM_ERR_INVALID_ARG;
    if (nsym > SIZE_MAX / 8) return MODEM_ERR_INVALID_ARG;
    const size_t nllr = nsym * h->bps;
    if (cap < nllr) return MODEM_ERR_CAPACITY;
    if (nsym == 0) return MODEM_OK;
    const PtrKind ki = ptr_kind(iq, h->device), ko = ptr_kind(llr, h->device);
    if (ki == PTR_FOREIGN || ko == PTR_FOREIGN) return MODEM_ERR_INVALID_ARG;
    const size_t in_bytes = nsym * (h->in_dtype == MODEM_DTYPE_F16 ? 4 : 8), ob = demap_out_bytes(h->out_dtype);
    // device pointers must be element-aligned (the kernel picks its access widths from there up)
    if ((ki == PTR_DEVICE && reinterpret_cast<uintptr_t>(iq) % (h->in_dtype == MODEM_DTYPE_F16 ? 2 : 4)) ||
        (ko == PTR_DEVICE && reinterpret_cast<uintptr_t>(llr) % ob)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    modem_status st;
    const void* din = iq;
    void* dout = llr;
    if (ki == PTR_HOST) {
        if ((st = h->in_stage.ensure(in_bytes))) return st;
        HIP_TRY(hipMemcpyAsync(h->in_stage.p, iq, in_bytes, hipMemcpyHostToDevice, s));
        din = h->in_stage.p;
    }
    const bool host_out = ko == PTR_HOST;
    if (host_out) {
        if ((st = h->out_stage.ensure(nllr * ob))) return st;
        dout = h->out_stage.p;
    }
    mk::DemapParams p{};
    p.iq = din;
    p.llr = dout;
    p.tab = h->d_tab;
    p.nsym = (int64_t)nsym;
    p.scale = scale;
    p.bps = (int32_t)h->bps;
    HIP_TRY(mk::launch_demap(p, h->axis, h->in_dtype, h->out_dtype, s));
    if (host_out) HIP_TRY(hipMemcpyAsync(llr, dout, nllr * ob, hipMemcpyDeviceToHost, s));
    if (host_out || din != iq) HIP_TRY(hipStreamSynchronize(s));
    return MODEM_OK;
}

int modem_demap_path(const modem_demap* h) { return h ? (h->axis ? 1 : 0) : -1; }

modem_status modem_demap_destroy(modem_demap* h) { delete h; return MODEM_OK; }

// ---------------------------------------------------------- noncoherent detectors ----
modem_status modem_phasor_diff_lut(const modem_phasor_desc* d, float* lut) {
    if (!d || !lut) return MODEM_ERR_INVALID_ARG;
    if (d->kind != MODEM_PHASOR_DMPSK) return MODEM_ERR_UNSUPPORTED;
    uint32_t bps = 0;
    modem_status st;
    if ((st = phasor_bps(d, &bps))) return st;
    for (uint32_t s = 0; s < (1u << bps); ++s) {
        const float a = (float)s * d->shift;                       // the product of dmpsk.rs:32
        lut[2 * s] = (float)std::cos((double)a);
        lut[2 * s + 1] = (float)std::sin((double)a);
    }
    return MODEM_OK;
}

modem_status modem_phasor_tones(const modem_phasor_desc* d, float carrier_sample_freq, float* omega) {
    if (!d || !omega) return MODEM_ERR_INVALID_ARG;
    if (d->kind != MODEM_PHASOR_MFSK && d->kind != MODEM_PHASOR_BFSK) return MODEM_ERR_UNSUPPORTED;
    uint32_t bps = 0;
    modem_status st;
    if ((st = phasor_bps(d, &bps))) return st;
    if (d->kind == MODEM_PHASOR_MFSK && d->mfsk_map > 1) return MODEM_ERR_INVALID_ARG;
    const int max_symbol = (1 << bps) - 1;
    for (int m = 0; m <= max_symbol; ++m) {
        const int coef = d->kind == MODEM_PHASOR_BFSK ? m               // bfsk.rs:27-29
                         : d->mfsk_map ? 2 * m                          // mfsk.rs:31-35
                                       : 2 * m - max_symbol;            // mfsk.rs:23-27
        omega[m] = (float)((double)carrier_sample_freq + (double)coef * (double)d->freq);
    }
    return MODEM_OK;
}

static bool llr_dtype_ok(int32_t dt) { return dt == MODEM_DTYPE_F32 || dt == MODEM_DTYPE_F16 || dt == MODEM_DTYPE_I8; }
static bool iq_dtype_ok(int32_t dt) { return dt == MODEM_DTYPE_F32 || dt == MODEM_DTYPE_F16; }

// Host / device I/O of one process() call: inputs staged before the launch, outputs after it.
struct NoncohIo {
    int device;
    hipStream_t s;
    bool sync = false;
    modem_status in(Stage& st, const void* p, size_t bytes, const void** dev) {
        *dev = p;
        if (!p || !bytes || ptr_kind(p, device) == PTR_DEVICE) return MODEM_OK;
        modem_status e;
        if ((e = st.ensure(bytes))) return e;
        HIP_TRY(hipMemcpyAsync(st.p, p, bytes, hipMemcpyHostToDevice, s));
        *dev = st.p;
        sync = true;
        return MODEM_OK;
    }
    modem_status out(Stage& st, void* p, size_t bytes, void** dev) {
        *dev = p;
        if (!p || !bytes || ptr_kind(p, device) == PTR_DEVICE) return MODEM_OK;
        modem_status e;
        if ((e = st.ensure(bytes))) return e;
        *dev = st.p;
        return MODEM_OK;
    }
    modem_status back(void* p, const void* dev, size_t bytes) {
        if (!p || !bytes || dev == p) return MODEM_OK;
        HIP_TRY(hipMemcpyAsync(p, dev, bytes, hipMemcpyDeviceToHost, s));
        sync = true;
        return MODEM_OK;
    }
    modem_status finish() {
        if (sync) HIP_TRY(hipStreamSynchronize(s));
        return MODEM_OK;
    }
};

// A device pointer must be element-aligned, and on the handle's device.
static bool noncoh_ptr_bad(const void* p, size_t align, int device) {
    const PtrKind k = ptr_kind(p, device);
    return k == PTR_FOREIGN || (k == PTR_DEVICE && reinterpret_cast<uintptr_t>(p) % align);
}

struct modem_diff {
    int device = 0;
    uint32_t bps = 0;
    int32_t in_dtype = 0, llr_dtype = 0;
    float* d_tab = nullptr;      // 2^bps (cos, sin) pairs
    float2* d_prev = nullptr;    // two slots: [cur] = the point before the next call's first
    int cur = 0;
    Stage in_stage, sym_stage, llr_stage;
    ~modem_diff() {
        DeviceGuard g(device);
        if (d_tab) (void)hipFree(d_tab);
        if (d_prev) (void)hipFree(d_prev);
    }
};

modem_status modem_diff_create(const float* lut, uint32_t bits_per_symbol, const float prev0[2], int32_t in_dtype,
                               int32_t llr_dtype, int device, modem_diff** out) {
    if (!out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (!lut || bits_per_symbol < 1 || bits_per_symbol > 8) return MODEM_ERR_INVALID_ARG;
    if (!iq_dtype_ok(in_dtype) || !llr_dtype_ok(llr_dtype)) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_diff* h = new (std::nothrow) modem_diff;
    if (!h) return MODEM_ERR_ALLOC;
    h->device = device;
    h->bps = bits_per_symbol;
    h->in_dtype = in_dtype;
    h->llr_dtype = llr_dtype;
    const size_t ntab = (size_t)2 << bits_per_symbol;
    const float prev[2] = {prev0 ? prev0[0] : 1.0f, prev0 ? prev0[1] : 0.0f};
    modem_status st;
    if ((st = dalloc(&h->d_tab, ntab)) || (st = dalloc(&h->d_prev, 2))) { delete h; return st; }
    if (hipMemcpy(h->d_tab, lut, ntab * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_prev, prev, sizeof(prev), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); delete h; return MODEM_ERR_HIP;
    }
    *out = h;
    return MODEM_OK;
}

modem_status modem_diff_process(modem_diff* h, const void* iq, size_t nsym, float scale, uint8_t* out_sym, void* llr,
                                size_t cap, void* stream) {
    if (!h || !std::isfinite(scale) || (nsym && !iq)) return MODEM_ERR_INVALID_ARG;
    if (nsym > SIZE_MAX / 32) return MODEM_ERR_INVALID_ARG;
    if (cap < nsym) return MODEM_ERR_CAPACITY;
    if (nsym == 0) return MODEM_OK;
    const size_t isz = h->in_dtype == MODEM_DTYPE_F16 ? 2 : 4, ob = demap_out_bytes(h->llr_dtype);
    if (noncoh_ptr_bad(iq, isz, h->device) || noncoh_ptr_bad(out_sym, 1, h->device) ||
        noncoh_ptr_bad(llr, ob, h->device)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    NoncohIo io{h->device, (hipStream_t)stream};
    const size_t llr_bytes = nsym * h->bps * ob;
    modem_status st;
    mk::DiffParams p{};
    void *dsym, *dllr;
    if ((st = io.in(h->in_stage, iq, nsym * 2 * isz, &p.iq)) || (st = io.out(h->sym_stage, out_sym, nsym, &dsym)) ||
        (st = io.out(h->llr_stage, llr, llr_bytes, &dllr))) return st;
    p.prev = h->d_prev + h->cur;
    p.prev_new = h->d_prev + (h->cur ^ 1);
    p.tab = h->d_tab;
    p.sym = static_cast<uint8_t*>(dsym);
    p.llr = dllr;
    p.nsym = (int64_t)nsym;
    p.scale = scale;
    p.bps = (int32_t)h->bps;
    HIP_TRY(mk::launch_diff(p, h->in_dtype, h->llr_dtype, io.s));
    h->cur ^= 1;
    if ((st = io.back(out_sym, dsym, nsym)) || (st = io.back(llr, dllr, llr_bytes))) return st;
    return io.finish();
}

modem_status modem_diff_destroy(modem_diff* h) { delete h; return MODEM_OK; }

struct modem_fsk {
    int device = 0;
    uint32_t bps = 0, sps = 0;
    int32_t in_dtype = 0, llr_dtype = 0;
    float2* d_tw = nullptr;      // sps * 2^bps twiddles, mk::fsk_tw_index order
    char* d_carry = nullptr;     // two buffers of sps samples of in_dtype: [cur] holds ncarry of them
    int cur = 0;
    uint32_t ncarry = 0;
    Stage in_stage, sym_stage, llr_stage, e_stage;
    size_t carry_bytes() const { return (size_t)sps * (in_dtype == MODEM_DTYPE_F16 ? 4 : 8); }
    ~modem_fsk() {
        DeviceGuard g(device);
        if (d_tw) (void)hipFree(d_tw);
        if (d_carry) (void)hipFree(d_carry);
    }
};

modem_status modem_fsk_create(const float* omega, uint32_t bits_per_symbol, uint32_t samples_per_symbol,
                              int32_t in_dtype, int32_t llr_dtype, int device, modem_fsk** out) {
    if (!out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (!omega || bits_per_symbol < 1 || bits_per_symbol > 8 || samples_per_symbol < 1) return MODEM_ERR_INVALID_ARG;
    if (!iq_dtype_ok(in_dtype) || !llr_dtype_ok(llr_dtype)) return MODEM_ERR_INVALID_ARG;
    const uint32_t M = 1u << bits_per_symbol, sps = samples_per_symbol;
    for (uint32_t m = 0; m < M; ++m)
        if (!std::isfinite(omega[m])) return MODEM_ERR_INVALID_ARG;
    if ((uint64_t)sps * M > 65536) return MODEM_ERR_UNSUPPORTED;    // the twiddle table: 512 KiB at most
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_fsk* h = new (std::nothrow) modem_fsk;
    if (!h) return MODEM_ERR_ALLOC;
    h->device = device;
    h->bps = bits_per_symbol;
    h->sps = sps;
    h->in_dtype = in_dtype;
    h->llr_dtype = llr_dtype;
    // e^{-j omega[m] i} as (cos, -sin): the angle is exact in double (24 x 16 bits), the values
    // are double libm's rounded to f32
    std::vector<float2> tw((size_t)sps * M);
    for (uint32_t m = 0; m < M; ++m)
        for (uint32_t i = 0; i < sps; ++i) {
            const double a = (double)omega[m] * (double)i;
            tw[mk::fsk_tw_index((int)bits_per_symbol, (int)sps, (int)m, (int)i)] =
                make_float2((float)std::cos(a), (float)-std::sin(a));
        }
    modem_status st;
    if ((st = dalloc(&h->d_tw, tw.size())) || (st = dalloc(&h->d_carry, 2 * h->carry_bytes()))) { delete h; return st; }
    if (hipMemcpy(h->d_tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); delete h; return MODEM_ERR_HIP;
    }
    *out = h;
    return MODEM_OK;
}

modem_status modem_fsk_process(modem_fsk* h, const void* in, size_t n, float scale, uint8_t* out_sym, void* llr,
                               float* energy, size_t cap, size_t* produced, void* stream) {
    if (produced) *produced = 0;
    if (!h || !std::isfinite(scale) || (n && !in)) return MODEM_ERR_INVALID_ARG;
    if (n > SIZE_MAX / 32) return MODEM_ERR_INVALID_ARG;
    const size_t total = (size_t)h->ncarry + n, nsym = total / h->sps, M = (size_t)1 << h->bps;
    if (nsym > cap) return MODEM_ERR_CAPACITY;
    if (n == 0) return MODEM_OK;
    const size_t isz = h->in_dtype == MODEM_DTYPE_F16 ? 2 : 4, ob = demap_out_bytes(h->llr_dtype);
    if (noncoh_ptr_bad(in, isz, h->device) || noncoh_ptr_bad(out_sym, 1, h->device) ||
        noncoh_ptr_bad(llr, ob, h->device) || noncoh_ptr_bad(energy, 4, h->device)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    NoncohIo io{h->device, (hipStream_t)stream};
    const size_t llr_bytes = nsym * h->bps * ob, e_bytes = nsym * M * sizeof(float);
    modem_status st;
    mk::FskParams p{};
    void *dsym, *dllr, *de;
    if ((st = io.in(h->in_stage, in, n * 2 * isz, &p.in)) || (st = io.out(h->sym_stage, out_sym, nsym, &dsym)) ||
        (st = io.out(h->llr_stage, llr, llr_bytes, &dllr)) || (st = io.out(h->e_stage, energy, e_bytes, &de))) return st;
    p.carry = h->d_carry + (size_t)h->cur * h->carry_bytes();
    p.carry_new = h->d_carry + (size_t)(h->cur ^ 1) * h->carry_bytes();
    p.tw = h->d_tw;
    p.sym = static_cast<uint8_t*>(dsym);
    p.llr = dllr;
    p.energy = static_cast<float*>(de);
    p.n = (int64_t)n;
    p.nsym = (int64_t)nsym;
    p.ncarry = (int32_t)h->ncarry;
    p.sps = (int32_t)h->sps;
    p.bps = (int32_t)h->bps;
    p.scale = scale;
    HIP_TRY(mk::launch_fsk(p, h->in_dtype, h->llr_dtype, io.s));
    h->ncarry = (uint32_t)(total - nsym * h->sps);
    if (h->ncarry) h->cur ^= 1;                                     // the carry kernel filled the other buffer
    if (produced) *produced = nsym;
    if ((st = io.back(out_sym, dsym, nsym)) || (st = io.back(llr, dllr, llr_bytes)) ||
        (st = io.back(energy, de, e_bytes))) return st;
    return io.finish();
}

modem_status modem_fsk_destroy(modem_fsk* h) { delete h; return MODEM_OK; }

// ------------------------------------------------------------------- channel model ----
// The fraction bits of 1 / (2 pi), most significant first (bit i, i >= 1, has the weight 2^-i):
// 1280 bits, enough for the window below at every double exponent.
static const uint64_t kInv2Pi[20] = {
    0x28BE60DB9391054AULL, 0x7F09D5F47D4D3770ULL, 0x36D8A5664F10E410ULL, 0x7F9458EAF7AEF158ULL,
    0x6DC91B8E909374B8ULL, 0x01924BBA82746487ULL, 0x3F877AC72C4A69CFULL, 0xBA208D7D4BAED121ULL,
    0x3A671C09AD17DF90ULL, 0x4E64758E60D4CE7DULL, 0x272117E2EF7E4A0EULL, 0xC7FE25FFF7816603ULL,
    0xFBCBC462D6829B47ULL, 0xDB4D9FB3C9F2C26DULL, 0xD3D18FD9A797FA8BULL, 0x5D49EEB1FAF97C5EULL,
    0xCF41CE7DE294A4BAULL, 0x9AFED7EC47E35742ULL, 0x1580CC11BF1EDAEAULL, 0xFC33EF0826BD0D87ULL,
};

// frac(v / (2 pi)) * 2^64, rounded to nearest and wrapped mod 2^64, for any finite double
// (Payne-Hanek: |v| = m 2^E with a 53-bit integer m; the bits of 1 / (2 pi) of weight >= 2^-E give
// whole turns and drop out, the next 192 decide the result, the rest is below 2^-75 of its unit).
static uint64_t chan_turns(double v) {
    if (v == 0.0) return 0;
    int e = 0;
    const uint64_t m = (uint64_t)std::ldexp(std::frexp(std::fabs(v), &e), 53);
    const long E = (long)e - 53;
    const auto bit = [](long i) -> uint64_t {
        return i < 1 || i > 64 * 20 ? 0 : (kInv2Pi[(i - 1) / 64] >> (63 - (i - 1) % 64)) & 1;
    };
    uint64_t w[3] = {0, 0, 0};                          // bits E+1 .. E+192, w[0] the top
    for (int j = 0; j < 192; ++j) w[j / 64] = (w[j / 64] << 1) | bit(E + 1 + j);
    const unsigned __int128 p0 = (unsigned __int128)m * w[0], p1 = (unsigned __int128)m * w[1],
                            p2 = (unsigned __int128)m * w[2];
    const unsigned __int128 mid = (unsigned __int128)(uint64_t)p1 + (uint64_t)(p2 >> 64);
    const uint64_t r = (uint64_t)p0 + (uint64_t)(p1 >> 64) + (uint64_t)(mid >> 64) + (((uint64_t)mid) >> 63);
    return v < 0 ? (uint64_t)0 - r : r;
}

static uint64_t chan_mix64(uint64_t z) {                // splitmix64's finaliser (prng_bits)
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static const uint64_t kChanGolden = 0x9E3779B97F4A7C15ULL;

// The handle owns no device memory until a host pointer needs staging: its whole state is host-side.
struct modem_chan {
    int device = 0;
    int32_t in_dtype = 0, out_dtype = 0;
    float gain = 1.f, sig = 0.f;
    uint64_t key = 0;            // mix(seed + GOLDEN)
    uint64_t step = 0, phase0 = 0;
    uint64_t n = 0;              // absolute index of the next input sample
    Stage in_stage, out_stage;
};

modem_status modem_chan_create(double gain, double phase, double cfo, double n0, uint64_t seed, uint64_t s0,
                               int32_t in_dtype, int32_t out_dtype, int device, modem_chan** out) {
    if (!out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (!std::isfinite(gain) || !std::isfinite(phase) || !std::isfinite(cfo)) return MODEM_ERR_INVALID_ARG;
    if (!std::isfinite(n0) || n0 < 0.0) return MODEM_ERR_INVALID_ARG;
    if (!iq_dtype_ok(in_dtype) || !iq_dtype_ok(out_dtype)) return MODEM_ERR_INVALID_ARG;
    if (device < 0) return MODEM_ERR_NO_DEVICE;
    modem_chan* h = new (std::nothrow) modem_chan;
    if (!h) return MODEM_ERR_ALLOC;
    h->device = device;
    h->in_dtype = in_dtype;
    h->out_dtype = out_dtype;
    h->gain = (float)gain;
    h->sig = (float)std::sqrt(n0);
    h->key = chan_mix64(seed + kChanGolden);
    h->step = chan_turns(cfo);
    h->phase0 = chan_turns(phase);
    h->n = s0;
    *out = h;
    return MODEM_OK;
}

modem_status modem_chan_set_n0(modem_chan* h, double n0) {
    if (!h || !std::isfinite(n0) || n0 < 0.0) return MODEM_ERR_INVALID_ARG;
    h->sig = (float)std::sqrt(n0);
    return MODEM_OK;
}

modem_status modem_chan_nco(const modem_chan* h, uint64_t* step, uint64_t* phase0) {
    if (!h) return MODEM_ERR_INVALID_ARG;
    if (step) *step = h->step;
    if (phase0) *phase0 = h->phase0;
    return MODEM_OK;
}

uint64_t modem_chan_sample(const modem_chan* h) { return h ? h->n : 0; }

modem_status modem_chan_process(modem_chan* h, const void* in, size_t n, void* out, size_t cap, void* stream) {
    if (!h || (n && (!in || !out))) return MODEM_ERR_INVALID_ARG;
    if (n > SIZE_MAX / 8 || (uint64_t)n > UINT64_MAX - h->n) return MODEM_ERR_INVALID_ARG;   // s0 + n passes 2^64
    if (cap < n) return MODEM_ERR_CAPACITY;
    if (n == 0) return MODEM_OK;
    const size_t isz = h->in_dtype == MODEM_DTYPE_F16 ? 2 : 4, osz = h->out_dtype == MODEM_DTYPE_F16 ? 2 : 4;
    const size_t in_bytes = n * 2 * isz, out_bytes = n * 2 * osz;
    const uintptr_t ia = reinterpret_cast<uintptr_t>(in), oa = reinterpret_cast<uintptr_t>(out);
    // in place (the same address and dtype) or disjoint
    if (!(ia == oa && isz == osz) && ia < oa + out_bytes && oa < ia + in_bytes) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    if (noncoh_ptr_bad(in, isz, h->device) || noncoh_ptr_bad(out, osz, h->device)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    NoncohIo io{h->device, (hipStream_t)stream};
    modem_status st;
    mk::ChanParams p{};
    void* dout;
    if ((st = io.in(h->in_stage, in, in_bytes, &p.in)) || (st = io.out(h->out_stage, out, out_bytes, &dout))) return st;
    p.out = dout;
    p.n = (int64_t)n;
    p.cnt0 = h->key + (h->n + 1) * kChanGolden;
    p.ph0 = h->phase0 + h->step * h->n;
    p.step = h->step;
    p.gain = h->gain;
    p.sig = h->sig;
    HIP_TRY(mk::launch_chan(p, h->sig != 0.f, h->step != 0 || h->phase0 != 0, h->in_dtype, h->out_dtype, io.s));
    h->n += n;
    if ((st = io.back(out, dout, out_bytes))) return st;
    return io.finish();
}

modem_status modem_chan_destroy(modem_chan* h) { delete h; return MODEM_OK; }

// ------------------------------------------------------------- carrier synchronizer ----
// Host side: the sizes and the slot indices; device side: the < B carried symbols (two slots, the
// apply kernel fills the other one) and {theta, Phi, d} of the last block (two slots likewise).
struct modem_sync {
    int device = 0;
    int32_t in_dtype = 0, out_dtype = 0;
    int32_t lm = 0, lb = 0, flat = 0;
    float nrm = 1.f;
    uint64_t ref = 0, phase0 = 0;
    char* d_carry = nullptr;
    uint64_t* d_state = nullptr;
    int ccur = 0, scur = 0;
    uint32_t ncarry = 0;
    bool first = true;           // no block completed yet
    uint64_t n = 0;              // input symbols taken so far
    Stage in_stage, out_stage;
    Workspace phi_ws, th_ws, q_ws;
    size_t ssz() const { return in_dtype == MODEM_DTYPE_F16 ? 4 : 8; }
    size_t slot_bytes() const { return ((size_t)1 << lb) * ssz(); }
    ~modem_sync() {
        DeviceGuard g(device);
        if (d_carry) (void)hipFree(d_carry);
        if (d_state) (void)hipFree(d_state);
    }
};

modem_status modem_sync_create(uint32_t power, uint32_t block, double norm, double ref_phase, double phase0,
                               uint32_t flags, int32_t in_dtype, int32_t out_dtype, int device, modem_sync** out) {
    if (!out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (power != 2 && power != 4 && power != 8) return MODEM_ERR_INVALID_ARG;
    if (block < 64 || block > 4096 || (block & (block - 1))) return MODEM_ERR_INVALID_ARG;
    if (!std::isfinite(norm) || !(norm > 0.0) || !std::isfinite(ref_phase) || !std::isfinite(phase0)) return MODEM_ERR_INVALID_ARG;
    if (flags & ~(uint32_t)MODEM_SYNC_FLAT) return MODEM_ERR_INVALID_ARG;
    if (!iq_dtype_ok(in_dtype) || !iq_dtype_ok(out_dtype)) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_sync* h = new (std::nothrow) modem_sync;
    if (!h) return MODEM_ERR_ALLOC;
    h->device = device;
    h->in_dtype = in_dtype;
    h->out_dtype = out_dtype;
    h->lm = power == 2 ? 1 : power == 4 ? 2 : 3;
    for (h->lb = 6; (1u << h->lb) < block; ++h->lb) {}
    h->flat = (flags & MODEM_SYNC_FLAT) ? 1 : 0;
    h->nrm = (float)norm;
    h->ref = chan_turns(ref_phase);
    h->phase0 = chan_turns(phase0);
    // theta_{-1} = phase0, Phi_{-1} = M phase0, d = 0: what flush uses when no block was completed
    const uint64_t st0[mk::kSyncState] = {h->phase0, h->phase0 << h->lm, 0};
    modem_status st;
    if ((st = dalloc(&h->d_carry, 2 * h->slot_bytes())) || (st = dalloc(&h->d_state, 2 * mk::kSyncState))) { delete h; return st; }
    if (hipMemcpy(h->d_state, st0, sizeof(st0), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); delete h; return MODEM_ERR_HIP;
    }
    *out = h;
    return MODEM_OK;
}

static void sync_fill(const modem_sync* h, mk::SyncParams& p) {
    p.carry = h->d_carry + (size_t)h->ccur * h->slot_bytes();
    p.carry_new = h->d_carry + (size_t)(h->ccur ^ 1) * h->slot_bytes();
    p.state = h->d_state + (size_t)h->scur * mk::kSyncState;
    p.state_new = h->d_state + (size_t)(h->scur ^ 1) * mk::kSyncState;
    p.ref = h->ref;
    p.nrm = h->nrm;
    p.ncarry = (int32_t)h->ncarry;
    p.lb = h->lb;
    p.lm = h->lm;
    p.first = h->first ? 1 : 0;
    p.flat = h->flat;
}

modem_status modem_sync_process(modem_sync* h, const void* iq, size_t nsym, void* out, size_t cap, uint64_t* theta,
                                float* quality, size_t est_cap, size_t* produced, size_t* blocks, void* stream) {
    if (produced) *produced = 0;
    if (blocks) *blocks = 0;
    if (!h || (nsym && !iq)) return MODEM_ERR_INVALID_ARG;
    if (nsym > SIZE_MAX / 32) return MODEM_ERR_INVALID_ARG;
    const size_t total = (size_t)h->ncarry + nsym, nb = total >> h->lb, nout = nb << h->lb;
    if (nout && !out) return MODEM_ERR_INVALID_ARG;
    if (cap < nout || ((theta || quality) && est_cap < nb)) return MODEM_ERR_CAPACITY;
    if (nsym == 0) return MODEM_OK;
    const size_t isz = h->in_dtype == MODEM_DTYPE_F16 ? 2 : 4, osz = h->out_dtype == MODEM_DTYPE_F16 ? 2 : 4;
    const size_t in_bytes = nsym * 2 * isz, out_bytes = nout * 2 * osz;
    const uintptr_t ia = reinterpret_cast<uintptr_t>(iq), oa = reinterpret_cast<uintptr_t>(out);
    // the output lags the input by the carried symbols: no in-place form, the byte ranges must be disjoint
    if (out_bytes && ia < oa + out_bytes && oa < ia + in_bytes) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    if (noncoh_ptr_bad(iq, isz, h->device) || noncoh_ptr_bad(out, osz, h->device) || noncoh_ptr_bad(theta, 8, h->device) ||
        noncoh_ptr_bad(quality, 4, h->device)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    NoncohIo io{h->device, (hipStream_t)stream};
    modem_status st;
    mk::SyncParams p{};
    void* dout;
    if ((st = io.in(h->in_stage, iq, in_bytes, &p.in)) || (st = io.out(h->out_stage, out, out_bytes, &dout))) return st;
    if ((st = h->phi_ws.ensure(nb * sizeof(uint64_t))) || (st = h->th_ws.ensure((nb + 1) * sizeof(uint64_t))) ||
        (st = h->q_ws.ensure(nb * sizeof(float)))) return st;
    sync_fill(h, p);
    p.out = nout ? dout : nullptr;
    p.phi = static_cast<uint64_t*>(h->phi_ws.p);
    p.th = static_cast<uint64_t*>(h->th_ws.p);
    p.q = static_cast<float*>(h->q_ws.p);
    p.n = (int64_t)nsym;
    p.nblk = (int64_t)nb;
    HIP_TRY(mk::launch_sync(p, h->in_dtype, h->out_dtype, io.s));
    h->ncarry = (uint32_t)(total - nout);
    h->ccur ^= 1;                                                   // the apply kernel filled the other carry slot
    h->n += nsym;
    if (nb) {
        h->scur ^= 1;
        h->first = false;
        if (theta) {
            HIP_TRY(hipMemcpyAsync(theta, p.th + 1, nb * sizeof(uint64_t), hipMemcpyDefault, io.s));
            if (ptr_kind(theta, h->device) == PTR_HOST) io.sync = true;
        }
        if (quality) {
            HIP_TRY(hipMemcpyAsync(quality, p.q, nb * sizeof(float), hipMemcpyDefault, io.s));
            if (ptr_kind(quality, h->device) == PTR_HOST) io.sync = true;
        }
    }
    if (produced) *produced = nout;
    if (blocks) *blocks = nb;
    if ((st = io.back(out, dout, out_bytes))) return st;
    return io.finish();
}

modem_status modem_sync_flush(modem_sync* h, void* out, size_t cap, size_t* produced, void* stream) {
    if (produced) *produced = 0;
    if (!h) return MODEM_ERR_INVALID_ARG;
    const size_t n = h->ncarry;
    if (n && !out) return MODEM_ERR_INVALID_ARG;
    if (cap < n) return MODEM_ERR_CAPACITY;
    if (n == 0) return MODEM_OK;
    const size_t osz = h->out_dtype == MODEM_DTYPE_F16 ? 2 : 4, out_bytes = n * 2 * osz;
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    if (noncoh_ptr_bad(out, osz, h->device)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    NoncohIo io{h->device, (hipStream_t)stream};
    modem_status st;
    mk::SyncParams p{};
    void* dout;
    if ((st = io.out(h->out_stage, out, out_bytes, &dout))) return st;
    sync_fill(h, p);
    p.out = dout;
    HIP_TRY(mk::launch_sync_flush(p, h->in_dtype, h->out_dtype, io.s));
    h->ncarry = 0;                                                  // at a block boundary again; theta and Phi stay
    if (produced) *produced = n;
    if ((st = io.back(out, dout, out_bytes))) return st;
    return io.finish();
}

uint64_t modem_sync_symbol(const modem_sync* h) { return h ? h->n : 0; }

modem_status modem_sync_destroy(modem_sync* h) { delete h; return MODEM_OK; }

// -------------------------------------------------------- symbol timing synchronizer ----
// Host side: the sizes and the slot indices; device side: the H = 2 span N + 1 samples of history
// followed by the < B N samples of the incomplete block (two slots, the apply kernel fills the
// other one) and {D, Phi, d} of the last block (two slots likewise).
struct modem_timing {
    int device = 0;
    int32_t in_dtype = 0, out_dtype = 0;
    int32_t ln = 0, lb = 0, span = 0, flat = 0;
    char* d_pre = nullptr;
    int64_t* d_state = nullptr;
    int pcur = 0, scur = 0;
    uint32_t ncarry = 0;         // samples of the incomplete block
    bool first = true;           // no block completed yet
    uint64_t n = 0;              // input samples taken so far
    Stage in_stage, out_stage;
    Workspace phi_ws, th_ws, q_ws;
    size_t ssz() const { return in_dtype == MODEM_DTYPE_F16 ? 4 : 8; }
    size_t hist() const { return 2 * (size_t)span * ((size_t)1 << ln) + 1; }
    size_t bn() const { return (size_t)1 << (lb + ln); }
    size_t slot_bytes() const { return (hist() + bn() + 3) / 4 * 4 * ssz(); }      // a multiple of 16
    ~modem_timing() {
        DeviceGuard g(device);
        if (d_pre) (void)hipFree(d_pre);
        if (d_state) (void)hipFree(d_state);
    }
};

modem_status modem_timing_create(uint32_t sps, uint32_t block, uint32_t span, double tau0, uint32_t flags,
                                 int32_t in_dtype, int32_t out_dtype, int device, modem_timing** out) {
    if (!out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (sps != 4 && sps != 8) return MODEM_ERR_INVALID_ARG;
    if (block < 32 || block > 4096 || (block & (block - 1))) return MODEM_ERR_INVALID_ARG;
    if (span < 1 || span > 16) return MODEM_ERR_INVALID_ARG;
    if (!std::isfinite(tau0) || !(std::fabs(tau0) <= (double)span)) return MODEM_ERR_INVALID_ARG;
    if (flags & ~(uint32_t)MODEM_TIMING_FLAT) return MODEM_ERR_INVALID_ARG;
    if (!iq_dtype_ok(in_dtype) || !iq_dtype_ok(out_dtype)) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_timing* h = new (std::nothrow) modem_timing;
    if (!h) return MODEM_ERR_ALLOC;
    h->device = device;
    h->in_dtype = in_dtype;
    h->out_dtype = out_dtype;
    h->ln = sps == 4 ? 2 : 3;
    for (h->lb = 5; (1u << h->lb) < block; ++h->lb) {}
    h->span = (int32_t)span;
    h->flat = (flags & MODEM_TIMING_FLAT) ? 1 : 0;
    // D_{-1} = rint(tau0 * 2^32), Phi_{-1} = its low 32 bits, d = 0: what flush uses when no block was completed
    const int64_t d0 = (int64_t)std::rint(tau0 * 4294967296.0);
    const int64_t st0[mk::kTimingState] = {d0, (int64_t)(uint32_t)d0, 0};
    modem_status st;
    if ((st = dalloc(&h->d_pre, 2 * h->slot_bytes())) || (st = dalloc(&h->d_state, 2 * mk::kTimingState))) { delete h; return st; }
    if (hipMemset(h->d_pre, 0, 2 * h->slot_bytes()) != hipSuccess ||                 // x[n] = 0 for n < 0
        hipMemcpy(h->d_state, st0, sizeof(st0), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); delete h; return MODEM_ERR_HIP;
    }
    *out = h;
    return MODEM_OK;
}

static void timing_fill(const modem_timing* h, mk::TimingParams& p) {
    p.pre = h->d_pre + (size_t)h->pcur * h->slot_bytes();
    p.pre_new = h->d_pre + (size_t)(h->pcur ^ 1) * h->slot_bytes();
    p.state = h->d_state + (size_t)h->scur * mk::kTimingState;
    p.state_new = h->d_state + (size_t)(h->scur ^ 1) * mk::kTimingState;
    p.npre = (int32_t)(h->hist() + h->ncarry);
    p.lb = h->lb;
    p.ln = h->ln;
    p.span = h->span;
    p.first = h->first ? 1 : 0;
    p.flat = h->flat;
}

modem_status modem_timing_process(modem_timing* h, const void* in, size_t n, void* out, size_t cap, int64_t* tau,
                                  float* quality, size_t est_cap, size_t* produced, size_t* blocks, void* stream) {
    if (produced) *produced = 0;
    if (blocks) *blocks = 0;
    if (!h || (n && !in)) return MODEM_ERR_INVALID_ARG;
    if (n > SIZE_MAX / 32) return MODEM_ERR_INVALID_ARG;
    const size_t total = (size_t)h->ncarry + n, nb = total >> (h->lb + h->ln), nout = nb << h->lb;
    if (nout && !out) return MODEM_ERR_INVALID_ARG;
    if (cap < nout || ((tau || quality) && est_cap < nb)) return MODEM_ERR_CAPACITY;
    if (n == 0) return MODEM_OK;
    const size_t isz = h->in_dtype == MODEM_DTYPE_F16 ? 2 : 4, osz = h->out_dtype == MODEM_DTYPE_F16 ? 2 : 4;
    const size_t in_bytes = n * 2 * isz, out_bytes = nout * 2 * osz;
    const uintptr_t ia = reinterpret_cast<uintptr_t>(in), oa = reinterpret_cast<uintptr_t>(out);
    // an output symbol gathers samples around its own position: no in-place form, the byte ranges must be disjoint
    if (out_bytes && ia < oa + out_bytes && oa < ia + in_bytes) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    if (noncoh_ptr_bad(in, isz, h->device) || noncoh_ptr_bad(out, osz, h->device) || noncoh_ptr_bad(tau, 8, h->device) ||
        noncoh_ptr_bad(quality, 4, h->device)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    NoncohIo io{h->device, (hipStream_t)stream};
    modem_status st;
    mk::TimingParams p{};
    void* dout;
    if ((st = io.in(h->in_stage, in, in_bytes, &p.in)) || (st = io.out(h->out_stage, out, out_bytes, &dout))) return st;
    if ((st = h->phi_ws.ensure(nb * sizeof(uint32_t))) || (st = h->th_ws.ensure((nb + 1) * sizeof(int64_t))) ||
        (st = h->q_ws.ensure(nb * sizeof(float)))) return st;
    timing_fill(h, p);
    p.out = nout ? dout : nullptr;
    p.phi = static_cast<uint32_t*>(h->phi_ws.p);
    p.th = static_cast<int64_t*>(h->th_ws.p);
    p.q = static_cast<float*>(h->q_ws.p);
    p.n = (int64_t)n;
    p.nblk = (int64_t)nb;
    HIP_TRY(mk::launch_timing(p, h->in_dtype, h->out_dtype, io.s));
    h->ncarry = (uint32_t)(total - (nb << (h->lb + h->ln)));
    h->pcur ^= 1;                                                   // the apply kernel filled the other slot
    h->n += n;
    if (nb) {
        h->scur ^= 1;
        h->first = false;
        if (tau) {
            HIP_TRY(hipMemcpyAsync(tau, p.th + 1, nb * sizeof(int64_t), hipMemcpyDefault, io.s));
            if (ptr_kind(tau, h->device) == PTR_HOST) io.sync = true;
        }
        if (quality) {
            HIP_TRY(hipMemcpyAsync(quality, p.q, nb * sizeof(float), hipMemcpyDefault, io.s));
            if (ptr_kind(quality, h->device) == PTR_HOST) io.sync = true;
        }
    }
    if (produced) *produced = nout;
    if (blocks) *blocks = nb;
    if ((st = io.back(out, dout, out_bytes))) return st;
    return io.finish();
}

modem_status modem_timing_flush(modem_timing* h, void* out, size_t cap, size_t* produced, void* stream) {
    if (produced) *produced = 0;
    if (!h) return MODEM_ERR_INVALID_ARG;
    const size_t nsym = h->ncarry >> h->ln;
    if (nsym && !out) return MODEM_ERR_INVALID_ARG;
    if (cap < nsym) return MODEM_ERR_CAPACITY;
    const size_t osz = h->out_dtype == MODEM_DTYPE_F16 ? 2 : 4, out_bytes = nsym * 2 * osz;
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    if (nsym && noncoh_ptr_bad(out, osz, h->device)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    NoncohIo io{h->device, (hipStream_t)stream};
    modem_status st;
    mk::TimingParams p{};
    void* dout;
    if ((st = io.out(h->out_stage, out, out_bytes, &dout))) return st;
    timing_fill(h, p);
    p.out = nsym ? dout : nullptr;
    p.nflush = (int32_t)nsym;
    HIP_TRY(mk::launch_timing_flush(p, h->in_dtype, h->out_dtype, io.s));
    h->ncarry = 0;                                                  // at a block boundary, the history all zero; D, Phi, d stay
    h->pcur ^= 1;
    if (produced) *produced = nsym;
    if ((st = io.back(out, dout, out_bytes))) return st;
    return io.finish();
}

uint64_t modem_timing_sample(const modem_timing* h) { return h ? h->n : 0; }

modem_status modem_timing_destroy(modem_timing* h) { delete h; return MODEM_OK; }

// ---------------------------------------------------------------- frame synchronizer ----
// Host side: the sizes, the slot index and the counters; device side: the unique word and the last
// min(T, 2W + L - 1) symbols of the window (two slots, the emit kernel fills the other one).
struct modem_frame {
    int device = 0;
    int32_t in_dtype = 0;
    int32_t L = 0, W = 0, maxh = 0;
    float t2 = 0.f, eu = 0.f;
    float* d_uw = nullptr;
    char* d_carry = nullptr;
    int ccur = 0;
    uint32_t ncarry = 0;
    uint64_t n = 0;              // input symbols taken so far
    Stage in_stage, pos_stage, phi_stage, met_stage, count_stage;
    Workspace cnt_ws, off_ws, rec_ws;
    size_t ssz() const { return in_dtype == MODEM_DTYPE_F16 ? 4 : 8; }
    size_t keep_max() const { return (size_t)(2 * W + L - 1); }
    size_t slot_bytes() const { return (keep_max() * ssz() + 15) / 16 * 16; }
    ~modem_frame() {
        DeviceGuard g(device);
        if (d_uw) (void)hipFree(d_uw);
        if (d_carry) (void)hipFree(d_carry);
    }
};

modem_status modem_frame_create(const float* uw, uint32_t len, uint32_t guard, double threshold, int32_t in_dtype,
                                int device, modem_frame** out) {
    if (!out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (!uw || len < 8 || len > (uint32_t)mk::kFrameMaxL || guard < 1 || guard > (uint32_t)mk::kFrameMaxW) return MODEM_ERR_INVALID_ARG;
    if (!std::isfinite(threshold) || !(threshold > 0.0) || !(threshold <= 1.0)) return MODEM_ERR_INVALID_ARG;
    if (!iq_dtype_ok(in_dtype)) return MODEM_ERR_INVALID_ARG;
    double eu = 0.0;
    for (uint32_t j = 0; j < len; ++j) {
        if (!std::isfinite(uw[2 * j]) || !std::isfinite(uw[2 * j + 1])) return MODEM_ERR_INVALID_ARG;
        eu += (double)uw[2 * j] * (double)uw[2 * j] + (double)uw[2 * j + 1] * (double)uw[2 * j + 1];
    }
    if (!(eu > 0.0) || !std::isfinite(eu)) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_frame* h = new (std::nothrow) modem_frame;
    if (!h) return MODEM_ERR_ALLOC;
    h->device = device;
    h->in_dtype = in_dtype;
    h->L = (int32_t)len;
    h->W = (int32_t)guard;
    h->maxh = (mk::kFrameTile + h->W) / (h->W + 1);
    h->t2 = (float)(threshold * threshold * eu);
    h->eu = (float)eu;
    modem_status st;
    if ((st = dalloc(&h->d_uw, 2 * (size_t)len)) || (st = dalloc(&h->d_carry, 2 * h->slot_bytes()))) { delete h; return st; }
    if (hipMemcpy(h->d_uw, uw, 2 * (size_t)len * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); delete h; return MODEM_ERR_HIP;
    }
    *out = h;
    return MODEM_OK;
}

static modem_status frame_run(modem_frame* h, const void* iq, size_t nsym, uint64_t* pos, uint32_t* phi, float* metric,
                              size_t cap, uint64_t* count, void* stream, bool flush) {
    if (!h || !pos || !count || (nsym && !iq)) return MODEM_ERR_INVALID_ARG;
    if (nsym > SIZE_MAX / 32) return MODEM_ERR_INVALID_ARG;
    const size_t isz = h->in_dtype == MODEM_DTYPE_F16 ? 2 : 4;
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    if (noncoh_ptr_bad(iq, isz, h->device) || noncoh_ptr_bad(pos, 8, h->device) || noncoh_ptr_bad(phi, 4, h->device) ||
        noncoh_ptr_bad(metric, 4, h->device) || noncoh_ptr_bad(count, 8, h->device)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    NoncohIo io{h->device, (hipStream_t)stream};
    modem_status st;
    mk::FrameParams p{};
    const int64_t nc = h->ncarry, nlog = nc + (int64_t)nsym, L = h->L, W = h->W;
    p.d0 = std::max<int64_t>(0, nc - W - L + 1);
    p.d1 = flush ? (nlog >= L ? nlog - L + 1 : 0) : std::max<int64_t>(0, nlog - W - L + 1);
    if (p.d1 < p.d0) p.d1 = p.d0;
    p.ntiles = (p.d1 - p.d0 + mk::kFrameTile - 1) / mk::kFrameTile;
    p.keep = flush ? 0 : (int32_t)std::min<int64_t>(nlog, (int64_t)h->keep_max());
    void *dpos, *dphi, *dmet, *dcount;
    if ((st = io.in(h->in_stage, iq, nsym * 2 * isz, &p.in)) || (st = io.out(h->pos_stage, pos, cap * 8, &dpos)) ||
        (st = io.out(h->phi_stage, phi, cap * 4, &dphi)) || (st = io.out(h->met_stage, metric, cap * 4, &dmet)) ||
        (st = io.out(h->count_stage, count, 8, &dcount))) return st;
    if ((st = h->cnt_ws.ensure((size_t)p.ntiles * sizeof(uint32_t))) || (st = h->off_ws.ensure((size_t)p.ntiles * sizeof(uint64_t))) ||
        (st = h->rec_ws.ensure((size_t)p.ntiles * h->maxh * 4 * sizeof(float)))) return st;
    p.carry = h->d_carry + (size_t)h->ccur * h->slot_bytes();
    p.carry_new = h->d_carry + (size_t)(h->ccur ^ 1) * h->slot_bytes();
    p.uw = h->d_uw;
    p.cnt = static_cast<uint32_t*>(h->cnt_ws.p);
    p.off = static_cast<uint64_t*>(h->off_ws.p);
    p.rec = static_cast<float*>(h->rec_ws.p);
    p.pos = static_cast<uint64_t*>(dpos);
    p.phi = static_cast<uint32_t*>(dphi);
    p.metric = static_cast<float*>(dmet);
    p.count = static_cast<uint64_t*>(dcount);
    p.n = (int64_t)nsym;
    p.base = h->n - (uint64_t)nc;
    p.cap = cap;
    p.t2 = h->t2;
    p.eu = h->eu;
    p.ncarry = (int32_t)nc;
    p.L = h->L;
    p.W = h->W;
    p.maxh = h->maxh;
    HIP_TRY(mk::launch_frame(p, h->in_dtype, io.s));
    h->ncarry = (uint32_t)p.keep;
    if (!flush) h->ccur ^= 1;                                       // the emit kernel filled the other carry slot
    h->n += nsym;
    if (dcount != count || dpos != pos || dphi != phi || dmet != metric) {
        // host outputs: the count first, then only the hits that were stored
        uint64_t got = 0;
        HIP_TRY(hipMemcpyAsync(&got, dcount, 8, hipMemcpyDeviceToHost, io.s));
        HIP_TRY(hipStreamSynchronize(io.s));
        if (dcount != count) *count = got;
        const size_t nw = (size_t)std::min<uint64_t>(got, cap);
        if ((st = io.back(pos, dpos, nw * 8)) || (st = io.back(phi, dphi, nw * 4)) || (st = io.back(metric, dmet, nw * 4))) return st;
    }
    return io.finish();
}

modem_status modem_frame_process(modem_frame* h, const void* iq, size_t nsym, uint64_t* pos, uint32_t* phi, float* metric,
                                 size_t cap, uint64_t* count, void* stream) {
    return frame_run(h, iq, nsym, pos, phi, metric, cap, count, stream, false);
}

modem_status modem_frame_flush(modem_frame* h, uint64_t* pos, uint32_t* phi, float* metric, size_t cap, uint64_t* count,
                               void* stream) {
    return frame_run(h, nullptr, 0, pos, phi, metric, cap, count, stream, true);
}

uint64_t modem_frame_symbol(const modem_frame* h) { return h ? h->n : 0; }

modem_status modem_frame_destroy(modem_frame* h) { delete h; return MODEM_OK; }

modem_status modem_frame_gather(const void* iq, size_t nsym, uint64_t base, const uint64_t* pos, const uint32_t* phi,
                                const uint64_t* count, size_t cap, uint32_t skip, uint32_t len, uint32_t power,
                                int32_t in_dtype, int32_t out_dtype, void* out, uint8_t* ok, int device, void* stream) {
    if (power != 1 && power != 2 && power != 4 && power != 8) return MODEM_ERR_INVALID_ARG;
    if (!iq_dtype_ok(in_dtype) || !iq_dtype_ok(out_dtype) || len == 0) return MODEM_ERR_INVALID_ARG;
    if ((nsym && !iq) || !count || (cap && (!pos || !out || !ok))) return MODEM_ERR_INVALID_ARG;
    if (nsym > SIZE_MAX / 32 || cap > SIZE_MAX / 32 / len) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    const size_t isz = in_dtype == MODEM_DTYPE_F16 ? 2 : 4, osz = out_dtype == MODEM_DTYPE_F16 ? 2 : 4;
    if (noncoh_ptr_bad(iq, isz, device) || noncoh_ptr_bad(pos, 8, device) || noncoh_ptr_bad(phi, 4, device) ||
        noncoh_ptr_bad(count, 8, device) || noncoh_ptr_bad(out, osz, device) || noncoh_ptr_bad(ok, 1, device)) return MODEM_ERR_INVALID_ARG;
    if (cap == 0) return MODEM_OK;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    NoncohIo io{device, (hipStream_t)stream};
    Stage s_in, s_pos, s_phi, s_count, s_out, s_ok;                // host memory: staged through buffers of this call, synchronous
    modem_status st;
    mk::FrameGatherParams p{};
    const void *dpos, *dphi, *dcount;
    void *dout, *dok;
    const size_t out_bytes = cap * len * 2 * osz;
    if ((st = io.in(s_in, iq, nsym * 2 * isz, &p.in)) || (st = io.in(s_pos, pos, cap * 8, &dpos)) ||
        (st = io.in(s_phi, phi, cap * 4, &dphi)) || (st = io.in(s_count, count, 8, &dcount)) ||
        (st = io.out(s_out, out, out_bytes, &dout)) || (st = io.out(s_ok, ok, cap, &dok))) return st;
    p.out = dout;
    p.ok = static_cast<uint8_t*>(dok);
    p.pos = static_cast<const uint64_t*>(dpos);
    p.phi = static_cast<const uint32_t*>(dphi);
    p.count = static_cast<const uint64_t*>(dcount);
    p.n = nsym;
    p.base = base;
    p.cap = cap;
    p.skip = skip;
    p.len = len;
    p.lm = power == 1 ? 0 : power == 2 ? 1 : power == 4 ? 2 : 3;
    HIP_TRY(mk::launch_frame_gather(p, in_dtype, out_dtype, io.s));
    if ((st = io.back(out, dout, out_bytes)) || (st = io.back(ok, dok, cap))) return st;
    return io.finish();
}

// ---------------------------------------------------------------- convolutional code ----
static bool conv_code_ok(uint32_t K, const uint32_t* polys, uint32_t n, uint32_t flags) {
    if (K < (uint32_t)mk::kFecMinK || K > (uint32_t)mk::kFecMaxK || (n != 2 && n != 3) || !polys) return false;
    if (flags & ~(uint32_t)MODEM_CONV_TAIL) return false;
    for (uint32_t j = 0; j < n; ++j)
        if (polys[j] == 0 || polys[j] >= (1u << K)) return false;
    return true;
}

// Device memory of `device`, aligned to its elements (every buffer of the code's entries).
static bool conv_ptr_bad(const void* p, size_t align, int device) {
    return ptr_kind(p, device) != PTR_DEVICE || reinterpret_cast<uintptr_t>(p) % align;
}

modem_status modem_conv_encode(uint32_t K, const uint32_t* polys, uint32_t n, uint32_t flags, const uint8_t* bits,
                               size_t nframes, size_t nbits, size_t in_stride, uint8_t* out, size_t out_stride, int device,
                               void* stream) {
    if (!conv_code_ok(K, polys, n, flags) || nbits == 0 || nbits > SIZE_MAX / 8 || in_stride < nbits) return MODEM_ERR_INVALID_ARG;
    const size_t T = nbits + ((flags & MODEM_CONV_TAIL) ? K - 1 : 0);
    if (out_stride / n < T || (nframes && (!bits || !out))) return MODEM_ERR_INVALID_ARG;
    if (nframes && (nframes > SIZE_MAX / in_stride || nframes > SIZE_MAX / out_stride)) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    if (nframes == 0) return MODEM_OK;
    if (conv_ptr_bad(bits, 1, device) || conv_ptr_bad(out, 1, device)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    mk::ConvEncodeParams p{};
    p.bits = bits;
    p.out = out;
    p.nframes = nframes;
    p.nbits = nbits;
    p.T = T;
    p.in_stride = in_stride;
    p.out_stride = out_stride;
    for (uint32_t j = 0; j < n; ++j) p.g[j] = polys[j];
    p.K = (int32_t)K;
    p.n = (int32_t)n;
    HIP_TRY(mk::launch_conv_encode(p, (hipStream_t)stream));
    return MODEM_OK;
}

// Host side: the code; device side: its S branch words, nothing that a call changes.
struct modem_viterbi {
    int device = 0;
    int32_t K = 0, n = 0, tail = 0, in_dtype = 0;
    uint32_t* d_table = nullptr;
    ~modem_viterbi() {
        DeviceGuard g(device);
        if (d_table) (void)hipFree(d_table);
    }
};

modem_status modem_viterbi_create(uint32_t K, const uint32_t* polys, uint32_t n, uint32_t flags, int32_t in_dtype, int device,
                                  modem_viterbi** out) {
    if (!out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (!conv_code_ok(K, polys, n, flags) || !llr_dtype_ok(in_dtype)) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_viterbi* h = new (std::nothrow) modem_viterbi;
    if (!h) return MODEM_ERR_ALLOC;
    h->device = device;
    h->K = (int32_t)K;
    h->n = (int32_t)n;
    h->tail = (flags & MODEM_CONV_TAIL) ? 1 : 0;
    h->in_dtype = in_dtype;
    const uint32_t S = 1u << (K - 1);
    std::vector<uint32_t> table(S);
    for (uint32_t s = 0; s < S; ++s) table[s] = mk::fec_branch_word(s, (int)K, polys, (int)n);
    modem_status st;
    if ((st = dalloc(&h->d_table, (size_t)S))) { delete h; return st; }
    if (hipMemcpy(h->d_table, table.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); delete h; return MODEM_ERR_HIP;
    }
    *out = h;
    return MODEM_OK;
}

modem_status modem_viterbi_process(modem_viterbi* h, const void* llr, size_t stride, size_t nframes, size_t nbits, float qscale,
                                   const uint8_t* ok, uint8_t* out, size_t out_stride, int32_t* metric, void* stream) {
    if (!h || nbits == 0 || !std::isfinite(qscale) || !(qscale > 0.0f)) return MODEM_ERR_INVALID_ARG;
    const size_t maxT = (size_t)mk::fec_max_steps(h->K), tailn = h->tail ? (size_t)(h->K - 1) : 0;
    if (nbits > maxT || nbits + tailn > maxT) return MODEM_ERR_INVALID_ARG;
    const size_t T = nbits + tailn, esz = demap_out_bytes(h->in_dtype);
    if (stride < (size_t)h->n * T || out_stride < nbits || (nframes && (!llr || !out))) return MODEM_ERR_INVALID_ARG;
    if (nframes && (nframes > SIZE_MAX / esz / stride || nframes > SIZE_MAX / out_stride)) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    if (nframes == 0) return MODEM_OK;
    if (conv_ptr_bad(llr, esz, h->device) || conv_ptr_bad(out, 1, h->device) || (ok && conv_ptr_bad(ok, 1, h->device)) ||
        (metric && conv_ptr_bad(metric, 4, h->device))) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    mk::ViterbiParams p{};
    p.llr = llr;
    p.ok = ok;
    p.table = h->d_table;
    p.out = out;
    p.metric = metric;
    p.nframes = nframes;
    p.stride = stride;
    p.out_stride = out_stride;
    p.qscale = qscale;
    p.K = h->K;
    p.n = h->n;
    p.tail = h->tail;
    p.nbits = (int32_t)nbits;
    p.T = (int32_t)T;
    HIP_TRY(mk::launch_viterbi(p, h->in_dtype, (hipStream_t)stream));
    return MODEM_OK;
}

modem_status modem_viterbi_destroy(modem_viterbi* h) { delete h; return MODEM_OK; }

modem_status modem_count_errors(const uint8_t* a, const uint8_t* b, size_t n, uint64_t* counts, int device, void* stream) {
    if (!counts || (n && (!a || !b))) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    const PtrKind kc = ptr_kind(counts, device);
    if (kc == PTR_FOREIGN || (kc == PTR_DEVICE && reinterpret_cast<uintptr_t>(counts) % 8)) return MODEM_ERR_INVALID_ARG;
    if (n && (ptr_kind(a, device) != kc || ptr_kind(b, device) != kc)) return MODEM_ERR_INVALID_ARG;   // all device or all host
    if (n == 0) return MODEM_OK;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (kc == PTR_DEVICE) {
        HIP_TRY(mk::launch_count_errors(a, b, n, counts, s));
        return MODEM_OK;
    }
    // host memory: staged through buffers of this call, synchronous
    Stage sa, sb, sc;
    modem_status st;
    if ((st = sa.ensure(n)) || (st = sb.ensure(n)) || (st = sc.ensure(2 * sizeof(uint64_t)))) return st;
    uint64_t got[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(sa.p, a, n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(sb.p, b, n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(sc.p, 0, sizeof(got), s));
    HIP_TRY(mk::launch_count_errors(static_cast<const uint8_t*>(sa.p), static_cast<const uint8_t*>(sb.p), n,
                                    static_cast<uint64_t*>(sc.p), s));
    HIP_TRY(hipMemcpyAsync(got, sc.p, sizeof(got), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    counts[0] += got[0];
    counts[1] += got[1];
    return MODEM_OK;
}

modem_status modem_prng_bits(uint64_t seed, uint8_t* out, size_t nbits, int device, void* stream) {
    if (nbits && !out) return MODEM_ERR_INVALID_ARG;
    if (nbits && (!is_device_ptr(out) || foreign_ptr(out, device))) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    HIP_TRY(mk::launch_prng_bits(seed, out, nbits, (hipStream_t)stream));
    return MODEM_OK;
}

}  // extern "C"
