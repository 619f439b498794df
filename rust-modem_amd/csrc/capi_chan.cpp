// rust-modem_amd/csrc/capi_chan.cpp — C ABI, host side: the channel model (its whole state is host-side).
#include "capi_common.h"
#include <cmath>

#pragma clang fp contract(off)

using namespace capi;

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
uint64_t capi::chan_turns(double v) {
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

extern "C" {

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
    const size_t isz = dtype_bytes(h->in_dtype), osz = dtype_bytes(h->out_dtype);
    const size_t in_bytes = n * 2 * isz, out_bytes = n * 2 * osz;
    const uintptr_t ia = reinterpret_cast<uintptr_t>(in), oa = reinterpret_cast<uintptr_t>(out);
    // in place (the same address and dtype) or disjoint
    if (!(ia == oa && isz == osz) && ia < oa + out_bytes && oa < ia + in_bytes) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    HostIo io{h->device, (hipStream_t)stream};
    IoPtr x(in), y(out);
    if (!io.take(x, isz) || !io.take(y, osz)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    mk::ChanParams p{};
    if ((st = io.in(x, h->in_stage, in_bytes)) || (st = io.out(y, h->out_stage, out_bytes))) return st;
    p.in = x.dev;
    p.out = y.dev;
    p.n = (int64_t)n;
    p.cnt0 = h->key + (h->n + 1) * kChanGolden;
    p.ph0 = h->phase0 + h->step * h->n;
    p.step = h->step;
    p.gain = h->gain;
    p.sig = h->sig;
    HIP_TRY(mk::launch_chan(p, h->sig != 0.f, h->step != 0 || h->phase0 != 0, h->in_dtype, h->out_dtype, io.s));
    h->n += n;
    if ((st = io.back(y, out_bytes))) return st;
    return io.finish();
}

modem_status modem_chan_destroy(modem_chan* h) { delete h; return MODEM_OK; }

}  // extern "C"
