// rust-modem_amd/csrc/capi_rx.cpp — C ABI, host side: the streaming RX handle (its tables, the
// per-call parameters, the state) and its batch entry.
#include "capi_handles.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

#pragma clang fp contract(off)

using namespace capi;

namespace capi {

// Kept instants n = k*decim + D with n in [a, b): first k and count.
void rx_range(int64_t a, int64_t b, int64_t decim, int64_t D, int64_t* k0, int64_t* cnt) {
    auto first_at_or_after = [&](int64_t n) -> int64_t {
        return n <= D ? 0 : (n - D + decim - 1) / decim;
    };
    *k0 = first_at_or_after(a);
    const int64_t k1 = first_at_or_after(b);
    *cnt = k1 > *k0 ? k1 - *k0 : 0;
}

// Kernel parameters of one RX call on device buffers; see rx_run.
void rx_fill(const modem_rx* h, const void* din, size_t n, void* diq, uint8_t* dsym, int64_t k_first, int64_t nout,
             mk::RxParams& p) {
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
void rx_advance(modem_rx* h, size_t n) {
    h->hcur ^= 1;
    h->consumed += (int64_t)n;
}

// The kernel launch of one RX call on device buffers and the handle's state update.
modem_status rx_launch(modem_rx* h, const void* din, size_t n, void* diq, uint8_t* dsym, int64_t k_first, int64_t nout,
                       hipStream_t s) {
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

}  // namespace capi

// `zeros`: the flush, n samples of the handle's zero buffer (nothing staged). `known`: the caller
// (the batch entry) has classified the three pointers already.
static modem_status rx_run(modem_rx* h, IoPtr x, size_t n, bool zeros, IoPtr iq, IoPtr sym, size_t cap, size_t* produced,
                           hipStream_t s, bool known = false) {
    if (!h || !produced || (n && !x.user && !zeros)) return MODEM_ERR_INVALID_ARG;
    *produced = 0;
    int64_t k_first, nout;
    rx_range(h->consumed, h->consumed + (int64_t)n, h->decim, h->D, &k_first, &nout);
    if ((size_t)nout > cap) return MODEM_ERR_CAPACITY;
    HostIo io{h->device, s};
    // (device pointers of any alignment; an empty buffer's pointer is not looked at)
    if (!known && ((n && !zeros && !io.take(x)) || (nout && (!io.take(iq) || !io.take(sym))))) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    if (zeros) x = IoPtr(h->d_zeros);
    const size_t iq_bytes = (size_t)nout * h->out_bytes();
    if ((st = io.in(x, h->in_stage, n * h->in_bytes())) || (st = io.out(iq, h->iq_stage, iq_bytes)) ||
        (st = io.out(sym, h->sym_stage, (size_t)nout))) return st;
    if ((st = rx_launch(h, x.dev, n, iq.dev, sym.as<uint8_t>(), k_first, nout, s))) return st;
    if ((st = io.back(iq, iq_bytes)) || (st = io.back(sym, (size_t)nout)) || (st = io.finish())) return st;
    *produced = (size_t)nout;
    return MODEM_OK;
}

extern "C" {

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
    NEW_HANDLE(modem_rx, h, device);
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
    const size_t esz = h->in_bytes();
    modem_status st;
    const auto bytes = [](void** p) { return reinterpret_cast<uint8_t**>(p); };
    const int ka_none[2] = {INT32_MIN, INT32_MIN};
    if ((st = upload(&h->d_taps, pp.data(), pp.size())) || (st = dalloc(&h->d_slut, 256)) ||
        (st = dalloc(bytes(&h->d_hist[0]), (h->HL + 1) * esz)) || (st = dalloc(bytes(&h->d_hist[1]), (h->HL + 1) * esz)) ||
        (st = dalloc(bytes(&h->d_zeros), (size_t)(h->ntaps) * esz)) || (st = upload(&h->d_ka, ka_none, 2)))
        return st;
    if (sl.kind == MODEM_SLICER_NEAREST && (st = h2d(h->d_slut, sl.lut, (size_t)1 << sl.bits_per_symbol))) return st;
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
        if ((st = dalloc(&h->d_bfrag, nfl))) return st;
        h->bfrag_host = tab;
        if ((st = h2d(reinterpret_cast<_Float16*>(h->d_bfrag), tab.data(), tab.size()))) return st;
    }
    *out = h.release();
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
    // every pointer classified once, for the refusal, the batch form and the single calls
    std::vector<IoPtr> px(ins, ins + nch), pq(out_iq, out_iq + nch), ps(out_sym, out_sym + nch);
    for (size_t c = 0; c < nch; ++c) {
        if (!hs[c]) continue;
        const HostIo io{hs[c]->device, s};
        if ((ns[c] && !io.take(px[c])) || !io.take(pq[c]) || !io.take(ps[c])) return MODEM_ERR_INVALID_ARG;
    }
    bool fuse = nch >= 2 && hs[0] != nullptr;
    for (size_t c = 0; fuse && c < nch; ++c) {
        const modem_rx* h = hs[c];
        const modem_rx* h0 = hs[0];
        fuse = h && h->device == h0->device && h->mfma_ksteps > 0 && h->mfma_ksteps == h0->mfma_ksteps &&
               h->mix == MODEM_MIX_COMPLEX && h->in_dtype == h0->in_dtype && h->out_dtype == h->in_dtype &&
               h->decim == h0->decim && h->ntaps == h0->ntaps && h->bfrag_host == h0->bfrag_host &&
               (ns[c] == 0 || (ins[c] && px[c].kind == PTR_DEVICE)) &&
               pq[c].kind == PTR_DEVICE && ps[c].kind == PTR_DEVICE;       // (a NULL output counts as device memory)
        for (size_t e = 0; fuse && e < c; ++e) fuse = hs[e] != h;
    }
    if (!fuse) {
        for (size_t c = 0; c < nch; ++c) {
            const modem_status st = rx_run(hs[c], px[c], ns[c], false, pq[c], ps[c], caps[c], &produced[c], s, true);
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

}  // extern "C"
