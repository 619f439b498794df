// rust-modem_amd/csrc/capi_timing.cpp — C ABI, host side: the feedforward symbol timing synchronizer.
#include "capi_common.h"
#include <cmath>

#pragma clang fp contract(off)

using namespace capi;

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
    size_t ssz() const { return 2 * dtype_bytes(in_dtype); }
    size_t hist() const { return 2 * (size_t)span * ((size_t)1 << ln) + 1; }
    size_t bn() const { return (size_t)1 << (lb + ln); }
    size_t slot_bytes() const { return (hist() + bn() + 3) / 4 * 4 * ssz(); }      // a multiple of 16
    ~modem_timing() {
        DeviceGuard g(device);
        if (d_pre) (void)hipFree(d_pre);
        if (d_state) (void)hipFree(d_state);
    }
};

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

extern "C" {

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
    NEW_HANDLE(modem_timing, h, device);
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
    if ((st = dalloc(&h->d_pre, 2 * h->slot_bytes())) || (st = dalloc(&h->d_state, 2 * mk::kTimingState))) return st;
    HIP_TRY(hipMemset(h->d_pre, 0, 2 * h->slot_bytes()));                            // x[n] = 0 for n < 0
    if ((st = h2d(h->d_state, st0, mk::kTimingState))) return st;
    *out = h.release();
    return MODEM_OK;
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
    const size_t isz = dtype_bytes(h->in_dtype), osz = dtype_bytes(h->out_dtype);
    const size_t in_bytes = n * 2 * isz, out_bytes = nout * 2 * osz;
    const uintptr_t ia = reinterpret_cast<uintptr_t>(in), oa = reinterpret_cast<uintptr_t>(out);
    // an output symbol gathers samples around its own position: no in-place form, the byte ranges must be disjoint
    if (out_bytes && ia < oa + out_bytes && oa < ia + in_bytes) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    HostIo io{h->device, (hipStream_t)stream};
    IoPtr x(in), y(out), th(tau), q(quality);
    if (!io.take(x, isz) || !io.take(y, osz) || !io.take(th, 8) || !io.take(q, 4)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    mk::TimingParams p{};
    if ((st = io.in(x, h->in_stage, in_bytes)) || (st = io.out(y, h->out_stage, out_bytes))) return st;
    if ((st = h->phi_ws.ensure(nb * sizeof(uint32_t))) || (st = h->th_ws.ensure((nb + 1) * sizeof(int64_t))) ||
        (st = h->q_ws.ensure(nb * sizeof(float)))) return st;
    timing_fill(h, p);
    p.in = x.dev;
    p.out = nout ? y.dev : nullptr;
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
        if (tau && (st = io.put(th, p.th + 1, nb * sizeof(int64_t)))) return st;
        if (quality && (st = io.put(q, p.q, nb * sizeof(float)))) return st;
    }
    if (produced) *produced = nout;
    if (blocks) *blocks = nb;
    if ((st = io.back(y, out_bytes))) return st;
    return io.finish();
}

modem_status modem_timing_flush(modem_timing* h, void* out, size_t cap, size_t* produced, void* stream) {
    if (produced) *produced = 0;
    if (!h) return MODEM_ERR_INVALID_ARG;
    const size_t nsym = h->ncarry >> h->ln;
    if (nsym && !out) return MODEM_ERR_INVALID_ARG;
    if (cap < nsym) return MODEM_ERR_CAPACITY;
    const size_t osz = dtype_bytes(h->out_dtype), out_bytes = nsym * 2 * osz;
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    HostIo io{h->device, (hipStream_t)stream};
    IoPtr y(out);
    if (nsym && !io.take(y, osz)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    mk::TimingParams p{};
    if ((st = io.out(y, h->out_stage, out_bytes))) return st;
    timing_fill(h, p);
    p.out = nsym ? y.dev : nullptr;
    p.nflush = (int32_t)nsym;
    HIP_TRY(mk::launch_timing_flush(p, h->in_dtype, h->out_dtype, io.s));
    h->ncarry = 0;                                                  // at a block boundary, the history all zero; D, Phi, d stay
    h->pcur ^= 1;
    if (produced) *produced = nsym;
    if ((st = io.back(y, out_bytes))) return st;
    return io.finish();
}

uint64_t modem_timing_sample(const modem_timing* h) { return h ? h->n : 0; }

modem_status modem_timing_destroy(modem_timing* h) { delete h; return MODEM_OK; }

}  // extern "C"
