// rust-modem_amd/csrc/capi_noncoh.cpp — C ABI, host side: the noncoherent detectors (differential PSK, FSK tone bank) and their tables.
#include "capi_common.h"
#include <cmath>

#pragma clang fp contract(off)

using namespace capi;

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

struct modem_fsk {
    int device = 0;
    uint32_t bps = 0, sps = 0;
    int32_t in_dtype = 0, llr_dtype = 0;
    float2* d_tw = nullptr;      // sps * 2^bps twiddles, mk::fsk_tw_index order
    char* d_carry = nullptr;     // two buffers of sps samples of in_dtype: [cur] holds ncarry of them
    int cur = 0;
    uint32_t ncarry = 0;
    Stage in_stage, sym_stage, llr_stage, e_stage;
    size_t carry_bytes() const { return (size_t)sps * 2 * dtype_bytes(in_dtype); }
    ~modem_fsk() {
        DeviceGuard g(device);
        if (d_tw) (void)hipFree(d_tw);
        if (d_carry) (void)hipFree(d_carry);
    }
};

extern "C" {

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

modem_status modem_diff_create(const float* lut, uint32_t bits_per_symbol, const float prev0[2], int32_t in_dtype,
                               int32_t llr_dtype, int device, modem_diff** out) {
    if (!out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (!lut || bits_per_symbol < 1 || bits_per_symbol > 8) return MODEM_ERR_INVALID_ARG;
    if (!iq_dtype_ok(in_dtype) || !llr_dtype_ok(llr_dtype)) return MODEM_ERR_INVALID_ARG;
    NEW_HANDLE(modem_diff, h, device);
    h->bps = bits_per_symbol;
    h->in_dtype = in_dtype;
    h->llr_dtype = llr_dtype;
    const size_t ntab = (size_t)2 << bits_per_symbol;
    const float prev[2] = {prev0 ? prev0[0] : 1.0f, prev0 ? prev0[1] : 0.0f};
    modem_status st;
    if ((st = upload(&h->d_tab, lut, ntab)) || (st = dalloc(&h->d_prev, 2)) || (st = h2d(h->d_prev, prev, 1))) return st;
    *out = h.release();
    return MODEM_OK;
}

modem_status modem_diff_process(modem_diff* h, const void* iq, size_t nsym, float scale, uint8_t* out_sym, void* llr,
                                size_t cap, void* stream) {
    if (!h || !std::isfinite(scale) || (nsym && !iq)) return MODEM_ERR_INVALID_ARG;
    if (nsym > SIZE_MAX / 32) return MODEM_ERR_INVALID_ARG;
    if (cap < nsym) return MODEM_ERR_CAPACITY;
    if (nsym == 0) return MODEM_OK;
    const size_t isz = dtype_bytes(h->in_dtype), ob = dtype_bytes(h->llr_dtype);
    HostIo io{h->device, (hipStream_t)stream};
    IoPtr x(iq), sym(out_sym), l(llr);
    if (!io.take(x, isz) || !io.take(sym, 1) || !io.take(l, ob)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    const size_t llr_bytes = nsym * h->bps * ob;
    modem_status st;
    mk::DiffParams p{};
    if ((st = io.in(x, h->in_stage, nsym * 2 * isz)) || (st = io.out(sym, h->sym_stage, nsym)) ||
        (st = io.out(l, h->llr_stage, llr_bytes))) return st;
    p.iq = x.dev;
    p.prev = h->d_prev + h->cur;
    p.prev_new = h->d_prev + (h->cur ^ 1);
    p.tab = h->d_tab;
    p.sym = sym.as<uint8_t>();
    p.llr = l.dev;
    p.nsym = (int64_t)nsym;
    p.scale = scale;
    p.bps = (int32_t)h->bps;
    HIP_TRY(mk::launch_diff(p, h->in_dtype, h->llr_dtype, io.s));
    h->cur ^= 1;
    if ((st = io.back(sym, nsym)) || (st = io.back(l, llr_bytes))) return st;
    return io.finish();
}

modem_status modem_diff_destroy(modem_diff* h) { delete h; return MODEM_OK; }

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
    NEW_HANDLE(modem_fsk, h, device);
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
    if ((st = upload(&h->d_tw, tw.data(), tw.size())) || (st = dalloc(&h->d_carry, 2 * h->carry_bytes()))) return st;
    *out = h.release();
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
    const size_t isz = dtype_bytes(h->in_dtype), ob = dtype_bytes(h->llr_dtype);
    HostIo io{h->device, (hipStream_t)stream};
    IoPtr x(in), sym(out_sym), l(llr), e(energy);
    if (!io.take(x, isz) || !io.take(sym, 1) || !io.take(l, ob) || !io.take(e, 4)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    const size_t llr_bytes = nsym * h->bps * ob, e_bytes = nsym * M * sizeof(float);
    modem_status st;
    mk::FskParams p{};
    if ((st = io.in(x, h->in_stage, n * 2 * isz)) || (st = io.out(sym, h->sym_stage, nsym)) ||
        (st = io.out(l, h->llr_stage, llr_bytes)) || (st = io.out(e, h->e_stage, e_bytes))) return st;
    p.in = x.dev;
    p.carry = h->d_carry + (size_t)h->cur * h->carry_bytes();
    p.carry_new = h->d_carry + (size_t)(h->cur ^ 1) * h->carry_bytes();
    p.tw = h->d_tw;
    p.sym = sym.as<uint8_t>();
    p.llr = l.dev;
    p.energy = e.as<float>();
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
    if ((st = io.back(sym, nsym)) || (st = io.back(l, llr_bytes)) || (st = io.back(e, e_bytes))) return st;
    return io.finish();
}

modem_status modem_fsk_destroy(modem_fsk* h) { delete h; return MODEM_OK; }

}  // extern "C"
