// rust-modem_amd/csrc/capi_tx.cpp — C ABI, host side: the streaming TX handle (its tables, the
// per-call parameters, the state) and its batch entry.
#include "capi_handles.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

#pragma clang fp contract(off)

using namespace capi;

namespace capi {

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
int64_t tx_nt_below(int64_t nsamp, uint64_t launch_bytes, bool single) {
    static const int mode = [] { const char* e = std::getenv("MODEM_TX_NT"); return e ? std::atoi(e) : 2; }();
    constexpr uint64_t kMin = 192ull << 20, kCache = 256ull << 20;
    if (mode == 0 || launch_bytes <= kMin || nsamp <= 0) return 0;
    // the cacheable second half pays only because the RX reads it first (mk::kRxTilesTopDown)
    return mode == 2 && single && mk::kRxTilesTopDown && launch_bytes <= kCache ? nsamp / 2 : nsamp;
}

// Kernel parameters of one TX call on device buffers (dbits, dout); see tx_run.
void tx_fill(const modem_tx* h, const uint8_t* dbits, size_t nbits, bool flush, void* dout, int64_t nsym,
             int ncarry_new, size_t nsamp, mk::TxParams& p) {
    p.bits = dbits;
    p.carry = h->d_carry[h->ccur];
    p.carry_new = h->d_carry[h->ccur ^ 1];
    p.hist = h->d_hist[h->hcur];
    p.hist_new = h->d_hist[h->hcur ^ 1];
    p.lut = h->d_lut;
    p.taps = h->d_taps;
    p.taps_q = h->d_taps_q;
    p.out = dout;
    p.nt_below = tx_nt_below((int64_t)nsamp, (uint64_t)nsamp * h->sample_bytes(), true);
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
void tx_advance(modem_tx* h, bool flush, int64_t nsym, int ncarry_new, size_t nsamp) {
    h->hcur ^= 1;
    if (!flush) { h->ccur ^= 1; h->ncarry = ncarry_new; }
    h->sample += nsamp;
    h->symbols += (uint64_t)nsym;
}

// The kernel launch of one TX call on device buffers and the handle's state update.
modem_status tx_launch(modem_tx* h, const uint8_t* dbits, size_t nbits, bool flush, void* dout, int64_t nsym,
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

}  // namespace capi

// `known`: the caller (the batch entry) has classified `b` and `o` already.
static modem_status tx_run(modem_tx* h, IoPtr b, size_t nbits, bool flush, IoPtr o, size_t cap, size_t* produced,
                           hipStream_t s, bool known = false) {
    if (!h || !produced || (nbits && !b.user)) return MODEM_ERR_INVALID_ARG;
    *produced = 0;
    const uint64_t total = (uint64_t)h->ncarry + nbits;
    const int64_t nsym = flush ? (int64_t)((h->ntaps ? h->ntaps - 1 + h->q_offset : 0) + h->sps - 1) / h->sps
                               : (int64_t)(total / h->bps);
    const int ncarry_new = flush ? h->ncarry : (int)(total - (uint64_t)nsym * h->bps);
    const size_t nsamp = (size_t)nsym * h->sps;
    if (nsamp > cap) return MODEM_ERR_CAPACITY;
    if (nsamp && !o.user) return MODEM_ERR_INVALID_ARG;
    HostIo io{h->device, s};
    // (device pointers of any alignment; an empty buffer's pointer is not looked at)
    if (!known && ((nbits && !io.take(b)) || (nsamp && !io.take(o)))) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    const size_t out_bytes = nsamp * h->sample_bytes();
    if ((st = io.in(b, h->bits_stage, nbits)) || (st = io.out(o, h->out_stage, out_bytes))) return st;
    if ((st = tx_launch(h, b.as<const uint8_t>(), nbits, flush, o.dev, nsym, ncarry_new, nsamp, s))) return st;
    // (host bits alone synchronise too: keep the caller's view simple)
    if ((st = io.back(o, out_bytes)) || (st = io.finish())) return st;
    *produced = nsamp;
    return MODEM_OK;
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

extern "C" {

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
    NEW_HANDLE(modem_tx, h, device);
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
    if ((st = lut_src ? upload(&h->d_lut, lut_src, nl) : dalloc(&h->d_lut, nl)) ||
        (st = upload(&h->d_taps, pp.data(), pp.size())) ||
        (st = dalloc(&h->d_hist[0], h->K)) || (st = dalloc(&h->d_hist[1], h->K)) ||
        (st = dalloc(&h->d_carry[0], 8)) || (st = dalloc(&h->d_carry[1], 8)) ||
        (D && (st = upload(&h->d_taps_q, pq.data(), pq.size()))))
        return st;
    // Sample-and-hold EvenOddOffset: before the first Q tick the phasor sees cur = [b0, 0]
    // (data.rs:84), i.e. the Q value of symbol index 0; it enters as the history symbol that
    // the delayed Q rail reads for n < D (its I value meets zero taps).
    // DMPSK starts from its phase (dmpsk.rs:20); MFSK / BFSK from zeros (mfsk.rs:55-56, bfsk.rs:16-17)
    if (pd && pd->kind == MODEM_PHASOR_DMPSK) {
        const float2 st0 = make_float2(pd->phase, 0.0f);
        if ((st = h2d(h->d_hist[0], &st0, 1))) return st;
    }
    if (D && d->ntaps == 0 && !pd && (st = h2d(h->d_hist[0] + (h->K - 2), d->lut, 1))) return st;
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
        if ((st = dalloc(&h->d_bfrag, nb)) || (st = dalloc(&h->d_luth, nlh))) return st;
        h->bfrag_host = bf;
        if ((st = h2d(reinterpret_cast<_Float16*>(h->d_bfrag), bf.data(), bf.size())) ||
            (st = h2d(reinterpret_cast<_Float16*>(h->d_luth), lh.data(), lh.size()))) return st;
    }
    *out = h.release();
    return MODEM_OK;
}

modem_status modem_tx_process(modem_tx* h, const uint8_t* bits, size_t nbits, void* out, size_t cap,
                              size_t* produced, void* stream) {
    return tx_run(h, bits, nbits, false, out, cap, produced, (hipStream_t)stream);
}
modem_status modem_tx_flush(modem_tx* h, void* out, size_t cap, size_t* produced, void* stream) {
    return tx_run(h, nullptr, 0, true, out, cap, produced, (hipStream_t)stream);
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
    // every pointer classified once, for the refusal, the two batch forms and the single calls
    // (an error leaves every handle untouched)
    std::vector<IoPtr> pb(bits, bits + nch), po(outs, outs + nch);
    for (size_t c = 0; c < nch; ++c) {
        if (!hs[c]) continue;
        const HostIo io{hs[c]->device, s};
        if ((nbits[c] && !io.take(pb[c])) || !io.take(po[c])) return MODEM_ERR_INVALID_ARG;
    }
    const auto on_device = [](const IoPtr& p) { return p.user && p.kind == PTR_DEVICE; };
    bool scan = nch >= 2 && hs[0] != nullptr && phasor_scanned(hs[0]->ph_kind);
    for (size_t c = 0; scan && c < nch; ++c) {
        const modem_tx* h = hs[c];
        // (a channel that completes no symbol writes no sample: its `out` may be NULL, as in tx_run)
        const bool writes = h && ((uint64_t)h->ncarry + nbits[c]) / h->bps > 0;
        scan = h && h->device == hs[0]->device && h->ph_kind == hs[0]->ph_kind &&
               (nbits[c] == 0 || on_device(pb[c])) && (writes ? on_device(po[c]) : !outs[c] || on_device(po[c]));
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
               h->bfrag_host == h0->bfrag_host && (nbits[c] == 0 || on_device(pb[c])) && on_device(po[c]);
        for (size_t e = 0; fuse && e < c; ++e) fuse = hs[e] != h;      // a handle at most once
    }
    if (!fuse) {
        for (size_t c = 0; c < nch; ++c) {
            const modem_status st = tx_run(hs[c], pb[c], nbits[c], false, po[c], caps[c], &produced[c], s, true);
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
            launch_bytes += (uint64_t)nsym[c0 + i] * hs[c0 + i]->sps * hs[c0 + i]->sample_bytes();
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

}  // extern "C"
