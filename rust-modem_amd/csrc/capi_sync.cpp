// rust-modem_amd/csrc/capi_sync.cpp — C ABI, host side: the feedforward carrier synchronizer.
#include "capi_common.h"
#include <cmath>

#pragma clang fp contract(off)

using namespace capi;

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
    size_t ssz() const { return 2 * dtype_bytes(in_dtype); }
    size_t slot_bytes() const { return ((size_t)1 << lb) * ssz(); }
    ~modem_sync() {
        DeviceGuard g(device);
        if (d_carry) (void)hipFree(d_carry);
        if (d_state) (void)hipFree(d_state);
    }
};

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

extern "C" {

modem_status modem_sync_create(uint32_t power, uint32_t block, double norm, double ref_phase, double phase0,
                               uint32_t flags, int32_t in_dtype, int32_t out_dtype, int device, modem_sync** out) {
    if (!out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (power != 2 && power != 4 && power != 8) return MODEM_ERR_INVALID_ARG;
    if (block < 64 || block > 4096 || (block & (block - 1))) return MODEM_ERR_INVALID_ARG;
    if (!std::isfinite(norm) || !(norm > 0.0) || !std::isfinite(ref_phase) || !std::isfinite(phase0)) return MODEM_ERR_INVALID_ARG;
    if (flags & ~(uint32_t)MODEM_SYNC_FLAT) return MODEM_ERR_INVALID_ARG;
    if (!iq_dtype_ok(in_dtype) || !iq_dtype_ok(out_dtype)) return MODEM_ERR_INVALID_ARG;
    NEW_HANDLE(modem_sync, h, device);
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
    if ((st = dalloc(&h->d_carry, 2 * h->slot_bytes())) || (st = dalloc(&h->d_state, 2 * mk::kSyncState)) ||
        (st = h2d(h->d_state, st0, mk::kSyncState))) return st;
    *out = h.release();
    return MODEM_OK;
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
    const size_t isz = dtype_bytes(h->in_dtype), osz = dtype_bytes(h->out_dtype);
    const size_t in_bytes = nsym * 2 * isz, out_bytes = nout * 2 * osz;
    const uintptr_t ia = reinterpret_cast<uintptr_t>(iq), oa = reinterpret_cast<uintptr_t>(out);
    // the output lags the input by the carried symbols: no in-place form, the byte ranges must be disjoint
    if (out_bytes && ia < oa + out_bytes && oa < ia + in_bytes) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    HostIo io{h->device, (hipStream_t)stream};
    IoPtr x(iq), y(out), th(theta), q(quality);
    if (!io.take(x, isz) || !io.take(y, osz) || !io.take(th, 8) || !io.take(q, 4)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    mk::SyncParams p{};
    if ((st = io.in(x, h->in_stage, in_bytes)) || (st = io.out(y, h->out_stage, out_bytes))) return st;
    if ((st = h->phi_ws.ensure(nb * sizeof(uint64_t))) || (st = h->th_ws.ensure((nb + 1) * sizeof(uint64_t))) ||
        (st = h->q_ws.ensure(nb * sizeof(float)))) return st;
    sync_fill(h, p);
    p.in = x.dev;
    p.out = nout ? y.dev : nullptr;
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
        if (theta && (st = io.put(th, p.th + 1, nb * sizeof(uint64_t)))) return st;
        if (quality && (st = io.put(q, p.q, nb * sizeof(float)))) return st;
    }
    if (produced) *produced = nout;
    if (blocks) *blocks = nb;
    if ((st = io.back(y, out_bytes))) return st;
    return io.finish();
}

modem_status modem_sync_flush(modem_sync* h, void* out, size_t cap, size_t* produced, void* stream) {
    if (produced) *produced = 0;
    if (!h) return MODEM_ERR_INVALID_ARG;
    const size_t n = h->ncarry;
    if (n && !out) return MODEM_ERR_INVALID_ARG;
    if (cap < n) return MODEM_ERR_CAPACITY;
    if (n == 0) return MODEM_OK;
    const size_t osz = dtype_bytes(h->out_dtype), out_bytes = n * 2 * osz;
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    HostIo io{h->device, (hipStream_t)stream};
    IoPtr y(out);
    if (!io.take(y, osz)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    mk::SyncParams p{};
    if ((st = io.out(y, h->out_stage, out_bytes))) return st;
    sync_fill(h, p);
    p.out = y.dev;
    HIP_TRY(mk::launch_sync_flush(p, h->in_dtype, h->out_dtype, io.s));
    h->ncarry = 0;                                                  // at a block boundary again; theta and Phi stay
    if (produced) *produced = n;
    if ((st = io.back(y, out_bytes))) return st;
    return io.finish();
}

uint64_t modem_sync_symbol(const modem_sync* h) { return h ? h->n : 0; }

modem_status modem_sync_destroy(modem_sync* h) { delete h; return MODEM_OK; }

}  // extern "C"
