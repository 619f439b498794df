// rust-modem_amd/csrc/capi_frame.cpp — C ABI, host side: the data-aided frame synchronizer and the frame gather.
#include "capi_common.h"
#include <cmath>

#pragma clang fp contract(off)

using namespace capi;

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
    size_t ssz() const { return 2 * dtype_bytes(in_dtype); }
    size_t keep_max() const { return (size_t)(2 * W + L - 1); }
    size_t slot_bytes() const { return (keep_max() * ssz() + 15) / 16 * 16; }
    ~modem_frame() {
        DeviceGuard g(device);
        if (d_uw) (void)hipFree(d_uw);
        if (d_carry) (void)hipFree(d_carry);
    }
};

static modem_status frame_run(modem_frame* h, const void* iq, size_t nsym, uint64_t* pos, uint32_t* phi, float* metric,
                              size_t cap, uint64_t* count, void* stream, bool flush) {
    if (!h || !pos || !count || (nsym && !iq)) return MODEM_ERR_INVALID_ARG;
    if (nsym > SIZE_MAX / 32) return MODEM_ERR_INVALID_ARG;
    const size_t isz = dtype_bytes(h->in_dtype);
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    HostIo io{h->device, (hipStream_t)stream};
    IoPtr x(iq), ps(pos), ph(phi), mt(metric), ct(count);
    if (!io.take(x, isz) || !io.take(ps, 8) || !io.take(ph, 4) || !io.take(mt, 4) || !io.take(ct, 8)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    mk::FrameParams p{};
    const int64_t nc = h->ncarry, nlog = nc + (int64_t)nsym, L = h->L, W = h->W;
    p.d0 = std::max<int64_t>(0, nc - W - L + 1);
    p.d1 = flush ? (nlog >= L ? nlog - L + 1 : 0) : std::max<int64_t>(0, nlog - W - L + 1);
    if (p.d1 < p.d0) p.d1 = p.d0;
    p.ntiles = (p.d1 - p.d0 + mk::kFrameTile - 1) / mk::kFrameTile;
    p.keep = flush ? 0 : (int32_t)std::min<int64_t>(nlog, (int64_t)h->keep_max());
    if ((st = io.in(x, h->in_stage, nsym * 2 * isz)) || (st = io.out(ps, h->pos_stage, cap * 8)) ||
        (st = io.out(ph, h->phi_stage, cap * 4)) || (st = io.out(mt, h->met_stage, cap * 4)) ||
        (st = io.out(ct, h->count_stage, 8))) return st;
    p.in = x.dev;
    if ((st = h->cnt_ws.ensure((size_t)p.ntiles * sizeof(uint32_t))) || (st = h->off_ws.ensure((size_t)p.ntiles * sizeof(uint64_t))) ||
        (st = h->rec_ws.ensure((size_t)p.ntiles * h->maxh * 4 * sizeof(float)))) return st;
    p.carry = h->d_carry + (size_t)h->ccur * h->slot_bytes();
    p.carry_new = h->d_carry + (size_t)(h->ccur ^ 1) * h->slot_bytes();
    p.uw = h->d_uw;
    p.cnt = static_cast<uint32_t*>(h->cnt_ws.p);
    p.off = static_cast<uint64_t*>(h->off_ws.p);
    p.rec = static_cast<float*>(h->rec_ws.p);
    p.pos = ps.as<uint64_t>();
    p.phi = ph.as<uint32_t>();
    p.metric = mt.as<float>();
    p.count = ct.as<uint64_t>();
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
    if (ct.staged() || ps.staged() || ph.staged() || mt.staged()) {
        // host outputs: the count first, then only the hits that were stored
        uint64_t got = 0;
        HIP_TRY(hipMemcpyAsync(&got, ct.dev, 8, hipMemcpyDeviceToHost, io.s));
        HIP_TRY(hipStreamSynchronize(io.s));
        if (ct.staged()) *count = got;
        const size_t nw = (size_t)std::min<uint64_t>(got, cap);
        if ((st = io.back(ps, nw * 8)) || (st = io.back(ph, nw * 4)) || (st = io.back(mt, nw * 4))) return st;
    }
    return io.finish();
}

extern "C" {

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
    NEW_HANDLE(modem_frame, h, device);
    h->in_dtype = in_dtype;
    h->L = (int32_t)len;
    h->W = (int32_t)guard;
    h->maxh = (mk::kFrameTile + h->W) / (h->W + 1);
    h->t2 = (float)(threshold * threshold * eu);
    h->eu = (float)eu;
    modem_status st;
    if ((st = upload(&h->d_uw, uw, 2 * (size_t)len)) || (st = dalloc(&h->d_carry, 2 * h->slot_bytes()))) return st;
    *out = h.release();
    return MODEM_OK;
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
    const size_t isz = dtype_bytes(in_dtype), osz = dtype_bytes(out_dtype);
    HostIo io{device, (hipStream_t)stream};
    IoPtr x(iq), ps(pos), ph(phi), ct(count), y(out), k(ok);
    if (!io.take(x, isz) || !io.take(ps, 8) || !io.take(ph, 4) || !io.take(ct, 8) || !io.take(y, osz) || !io.take(k, 1))
        return MODEM_ERR_INVALID_ARG;
    if (cap == 0) return MODEM_OK;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    Stage s_in, s_pos, s_phi, s_count, s_out, s_ok;                // host memory: staged through buffers of this call, synchronous
    modem_status st;
    mk::FrameGatherParams p{};
    const size_t out_bytes = cap * len * 2 * osz;
    if ((st = io.in(x, s_in, nsym * 2 * isz)) || (st = io.in(ps, s_pos, cap * 8)) || (st = io.in(ph, s_phi, cap * 4)) ||
        (st = io.in(ct, s_count, 8)) || (st = io.out(y, s_out, out_bytes)) || (st = io.out(k, s_ok, cap))) return st;
    p.in = x.dev;
    p.out = y.dev;
    p.ok = k.as<uint8_t>();
    p.pos = ps.as<const uint64_t>();
    p.phi = ph.as<const uint32_t>();
    p.count = ct.as<const uint64_t>();
    p.n = nsym;
    p.base = base;
    p.cap = cap;
    p.skip = skip;
    p.len = len;
    p.lm = power == 1 ? 0 : power == 2 ? 1 : power == 4 ? 2 : 3;
    HIP_TRY(mk::launch_frame_gather(p, in_dtype, out_dtype, io.s));
    if ((st = io.back(y, out_bytes)) || (st = io.back(k, cap))) return st;
    return io.finish();
}

}  // extern "C"
