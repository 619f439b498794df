// rust-modem_amd/csrc/capi_fir.cpp — C ABI, host side: the streaming FIR handle.
#include "capi_common.h"

using namespace capi;

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

extern "C" {

modem_status modem_fir_create(const float* taps, uint32_t ntaps, int device, modem_fir** out) {
    // FIRFilter::new(&[]) would divide by zero in add() (fir.rs:31): reject it here.
    if (!out || !taps || ntaps < 1 || ntaps > (uint32_t)mk::kMaxTaps) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    NEW_HANDLE(modem_fir, h, device);
    h->L = ntaps;
    modem_status st;
    if ((st = upload(&h->d_taps, taps, ntaps)) || (st = dalloc(&h->d_hist[0], ntaps)) ||
        (st = dalloc(&h->d_hist[1], ntaps))) return st;
    *out = h.release();
    return MODEM_OK;
}

modem_status modem_fir_process(modem_fir* h, const float* in, float* out, size_t n, void* stream) {
    if (!h || (n && (!in || !out))) return MODEM_ERR_INVALID_ARG;
    HostIo io{h->device, (hipStream_t)stream};
    IoPtr x(in), y(out);
    if (n && (!io.take(x) || !io.take(y))) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    if ((st = io.in(x, h->in_stage, n * sizeof(float))) || (st = io.out(y, h->out_stage, n * sizeof(float)))) return st;
    mk::FirParams p{};
    p.x = x.as<const float>();
    p.hist = h->d_hist[h->hcur];
    p.hist_new = h->d_hist[h->hcur ^ 1];
    p.y = y.as<float>();
    p.taps = h->d_taps;
    p.N = (int64_t)n;
    p.L = (int)h->L;
    HIP_TRY(mk::launch_fir(p, io.s));
    h->hcur ^= 1;
    if ((st = io.back(y, n * sizeof(float)))) return st;
    return io.finish();
}

modem_status modem_fir_destroy(modem_fir* h) { delete h; return MODEM_OK; }

}  // extern "C"
