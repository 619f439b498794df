// rust-modem_amd/csrc/capi_chain.cpp — C ABI, host side: prepared TX -> RX steps over fixed device buffers, one channel or a bank.
#include "capi_handles.h"
#include <cstdio>
#include <cstdlib>

using namespace capi;

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
            launch_bytes += (uint64_t)ns * t->sample_bytes();
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

extern "C" {

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

}  // extern "C"
