// rust-modem_amd/csrc/capi_handles.h — the TX and RX handles and the per-call pieces that the chain
// plans (capi_chain.cpp) share with capi_tx.cpp and capi_rx.cpp. Not part of the ABI.
#pragma once
#include "capi_common.h"

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
    capi::Workspace scan_stage;           // per-symbol states of the scanned phasors
    size_t scan_n = 0;              // symbols of the last call, in scan_stage (modem_tx_scan_states)
    int scan_path = 0;              // how the last call scanned them (modem_tx_scan_path)
    capi::Workspace batch_params;         // a scan batch's parameter blocks, when this is its first handle
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
    capi::Stage bits_stage, out_stage;
    size_t sample_bytes() const { return (out_mode == MODEM_OUT_REAL ? 1 : 2) * capi::dtype_bytes(dtype); }
    ~modem_tx() {
        capi::DeviceGuard g(device);
        for (void* p : {(void*)d_lut, (void*)d_taps, (void*)d_taps_q, (void*)d_hist[0], (void*)d_hist[1],
                        (void*)d_carry[0], (void*)d_carry[1], (void*)d_bfrag, (void*)d_luth})
            if (p) (void)hipFree(p);
    }
};

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
    capi::Stage in_stage, iq_stage, sym_stage;
    // one input sample (real int16 or an I/Q pair), one output point
    size_t in_bytes() const { return (in_dtype == MODEM_DTYPE_I16 ? 1 : 2) * capi::dtype_bytes(in_dtype); }
    size_t out_bytes() const { return 2 * capi::dtype_bytes(out_dtype); }
    ~modem_rx() {
        capi::DeviceGuard g(device);
        for (void* p : {(void*)d_taps, (void*)d_slut, d_hist[0], d_hist[1], d_zeros, (void*)d_bfrag, (void*)d_ka})
            if (p) (void)hipFree(p);
    }
};

namespace capi {

// capi_tx.cpp: the kernel parameters of one TX call on device buffers, the handle's state after it,
// the launch with that update, and the non-temporal store split of a launch (returns nt_below)
void tx_fill(const modem_tx* h, const uint8_t* dbits, size_t nbits, bool flush, void* dout, int64_t nsym,
             int ncarry_new, size_t nsamp, mk::TxParams& p);
void tx_advance(modem_tx* h, bool flush, int64_t nsym, int ncarry_new, size_t nsamp);
modem_status tx_launch(modem_tx* h, const uint8_t* dbits, size_t nbits, bool flush, void* dout, int64_t nsym,
                       int ncarry_new, size_t nsamp, hipStream_t s);
int64_t tx_nt_below(int64_t nsamp, uint64_t launch_bytes, bool single);

// capi_rx.cpp: the kept instants n = k*decim + D with n in [a, b) (first k and count), and the
// same pieces of one RX call
void rx_range(int64_t a, int64_t b, int64_t decim, int64_t D, int64_t* k0, int64_t* cnt);
void rx_fill(const modem_rx* h, const void* din, size_t n, void* diq, uint8_t* dsym, int64_t k_first, int64_t nout,
             mk::RxParams& p);
void rx_advance(modem_rx* h, size_t n);
modem_status rx_launch(modem_rx* h, const void* din, size_t n, void* diq, uint8_t* dsym, int64_t k_first, int64_t nout,
                       hipStream_t s);

}  // namespace capi
