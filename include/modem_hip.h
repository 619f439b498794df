/*
 * include/modem_hip.h — C ABI of the MI355X (gfx950) modem sample-path backend.
 *
 * This is the drop-in boundary for the hot path of ramtej/rust-modem (`src/modem`):
 *   bits -> symbol index -> (I,Q) LUT -> zero-stuff + RRC pulse-shaping FIR -> carrier mix
 *   -> [HBM sample buffer] -> conjugate mix -> matched filter at the decimated instants
 *   -> hard decision.
 * Every entry point is plain C: pointers, sizes, enums; no HIP or torch types (streams are
 * passed as an opaque `void*` hipStream_t; NULL = the device's default stream), so a Rust
 * `extern "C"` block, cgo or ctypes can bind it directly.
 *
 * Which reference interface each entry replaces (paths relative to the reference crate):
 *   modem_freq_sample_freq   freq.rs:19-26           Freq::new(hz, sr).sample_freq()
 *   modem_rates_sps          rates.rs:12-18          Rates::new(br, sr).samples_per_symbol
 *   modem_carrier_phase      carrier.rs:17-26,       Carrier::inner(s) = mod_trig(w * s as f32)
 *                            util.rs:3-6
 *   modem_phasor_lut         digital/phasor.rs:1-12, the memoryless DigitalPhasor plugins
 *                            bpsk.rs, qpsk.rs, qam.rs, bask.rs, mpsk.rs, apsk.rs, oqpsk.rs
 *   modem_tx_*               modulator.rs:64-101     DigitalModulator::new(&mut Carrier,
 *                            (+ fir.rs:3-35 for the   Box<DigitalPhasor>, Box<Source>) +
 *                            pulse shaping)           Iterator<Item=IQSample>; IQSample::
 *                                                     modulate (modulator.rs:45-48)
 *   modem_rx_*               demodulator.rs:7-56     Demodulator::new(Carrier, S, Fn()->
 *                                                     FIRFilter) + Iterator<Item=(f32,f32)>
 *   modem_fir_*              fir.rs:3-35             FIRFilter::new(&[f32]) + add(f32)->f32
 *   modem_chain_*            modulator.rs:85-100 then  one period of the sample-buffer loop:
 *                            demodulator.rs:44-56      the DigitalModulator's samples of a bit
 *                                                      buffer, then the Demodulator over them
 *   modem_chain_batch_*      the same, per channel       one period of a bank of independent
 *                                                      channels (one modulator and one
 *                                                      demodulator per stream)
 *
 * Conventions
 *   - Every function returns modem_status (0 = OK, negative = error) and never aborts.
 *     Where the reference panics (assert!, unwrap, out-of-range), this ABI returns
 *     MODEM_ERR_INVALID_ARG instead.
 *   - Taps and LUTs are copied at create time; the caller may free them afterwards.
 *   - I/O buffers are caller-owned. `*_process` accepts device pointers (asynchronous on
 *     `stream`) or host pointers (staged through the handle's device buffers; the call then
 *     synchronises `stream` before returning so the host buffers are valid).
 *   - Streaming: consecutive `*_process` calls equal one long call (the handle carries the
 *     carrier sample counter, the FIR history, leftover bits and the decimation phase);
 *     `*_flush` drains the filter with zeros.
 *   - Streams: a call whose buffers are all device memory queues everything it does (kernels,
 *     copies) on `stream` alone, in order, returns without waiting for the device and reads
 *     nothing back (tests/test_gpu_streams.py). The calls that wait for `stream` are those
 *     with a host pointer among their buffers, modem_tx_scan_states, and modem_count_errors on
 *     host memory; `*_create` copies tables with blocking copies and `*_destroy` frees device
 *     memory, which waits for the whole device: destroy a handle once its stream has drained.
 *     One handle, one stream at a time: a call reads the device state the previous call of
 *     that handle wrote, so consecutive calls go to one stream, or the caller orders the two
 *     streams with an event. Distinct handles share no device state and may run on distinct
 *     streams at once. Workspaces whose size follows the call (the per-symbol states of a
 *     DMPSK / MFSK / BFSK modem_tx, the per-block estimates of modem_sync and modem_timing,
 *     the per-tile tables of modem_frame) are allocated by the first call that needs them and
 *     grown, at least doubling, by a larger one; growing allocates and never frees: an
 *     outgrown buffer, which queued kernels may still use, lives until the handle is
 *     destroyed (all of them together are smaller than the live one).
 *   - One handle = one device; a handle is not thread-safe (it mirrors `&mut self`);
 *     distinct handles may be driven from different host threads. Device buffers passed to
 *     a handle must live on that handle's device (another GPU's memory: INVALID_ARG).
 */
#ifndef MODEM_HIP_H
#define MODEM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: modem_tx_desc.q_offset; 3: the channel-batch entry points; 4: modem_rx_desc.phase_offset
 * (the descriptor grew 8 bytes: 80 -> 88), modem_pll_lock, MODEM_DTYPE_I16 and
 * MODEM_MIX_REFERENCE_REAL_EXACT; 5: modem_chain_* (no layout change; modem_chain_fused
 * added later, additive); 6: modem_chain_batch_* (additive, no layout change; modem_demap_* and
 * MODEM_DTYPE_I8 added later, additive: no descriptor, no layout change; modem_tx_scan_states
 * and modem_tx_scan_path likewise; modem_phasor_diff_lut, modem_phasor_tones, modem_diff_* and
 * modem_fsk_* likewise; modem_chan_* and modem_count_errors likewise;
 * modem_sync_* likewise). Layouts: INTEGRATION.md. */
#define MODEM_HIP_ABI_VERSION 6

typedef enum {
    MODEM_OK = 0,
    MODEM_ERR_INVALID_ARG = -1,   /* the reference would panic (assert!/unwrap/index) */
    MODEM_ERR_UNSUPPORTED = -2,   /* outside what this backend implements */
    MODEM_ERR_HIP = -3,           /* a HIP runtime call failed */
    MODEM_ERR_NO_DEVICE = -4,     /* no gfx950 device / bad device ordinal */
    MODEM_ERR_CAPACITY = -5,      /* output buffer too small for the call */
    MODEM_ERR_ALLOC = -6          /* host or device allocation failed */
} modem_status;

/* I16: real-valued samples, one native-endian int16 per sample (what `demodulate` reads from
 * stdin, bin/util.rs:3-37); RX input only, with MODEM_MIX_REFERENCE_REAL_EXACT. */
/* I8: one signed byte per value; only as an LLR output dtype (modem_demap_create,
 * modem_diff_create, modem_fsk_create), every other entry point rejects it. */
typedef enum { MODEM_DTYPE_F32 = 0, MODEM_DTYPE_F16 = 1, MODEM_DTYPE_I16 = 2, MODEM_DTYPE_I8 = 3 } modem_dtype;

/* TX output: complex (i,q)*e^{j phase} (IQSample::modulate, modulator.rs:45-48); the
 * un-mixed baseband (what `modulate --iq` writes, modulate.rs:110-113); or only the real
 * part (what `modulate` writes by default, modulate.rs:128-133). */
typedef enum {
    MODEM_OUT_IQ_MIXED = 0,
    MODEM_OUT_IQ_BASEBAND = 1,
    MODEM_OUT_REAL = 2
} modem_out_mode;

/* RX mix: complex conjugate x*e^{-j phase} (loopback contract), or the reference's
 * real-input mix x.re*(cos, -sin) with the 2x gain (demodulator.rs:46,52-55). REAL_EXACT is
 * the latter with every f32 operation of the reference in its order: glibc's cosf / sinf
 * results (the libm Rust's f32::cos / sin call on x86-64 Linux), the products, and
 * FIRFilter::add's sequential fold (fir.rs:18-34) — outputs bit-identical to Demodulator's
 * (demodulator.rs:44-56). A VALU kernel: for the text front-end, not for throughput. */
typedef enum { MODEM_MIX_COMPLEX = 0, MODEM_MIX_REFERENCE_REAL = 1, MODEM_MIX_REFERENCE_REAL_EXACT = 2 } modem_mix;

typedef enum {
    MODEM_SLICER_NONE = 0,        /* no decisions */
    MODEM_SLICER_NEAREST = 1,     /* argmin |r - lut[s]|^2, lowest index on ties */
    MODEM_SLICER_QAM_AXIS = 2     /* per-axis round+clamp, for QAM at phase 0 */
} modem_slicer_kind;

/* ---- memoryless DigitalPhasor plugins (host-side LUT builders) -------------------------- */
typedef enum {
    MODEM_PHASOR_BPSK = 1,   /* BPSK::new(phase, amplitude)            bpsk.rs:10-15 */
    MODEM_PHASOR_QPSK = 2,   /* QPSK::new(phase, amplitude)            qpsk.rs:11-17 */
    MODEM_PHASOR_QAM = 3,    /* QAM::new(bits_per_symbol, phase, amp)  qam.rs:15-30 */
    MODEM_PHASOR_BASK = 4,   /* BASK::new(amplitude)                   bask.rs:8-12 */
    MODEM_PHASOR_MPSK = 5,   /* MPSK::new(bps, phase_offset, amp)      mpsk.rs:14-21 */
    MODEM_PHASOR_APSK = 6,   /* APSK::new(amplitude, bps, rings)       apsk.rs:25-33 */
    MODEM_PHASOR_OQPSK = 7,  /* OQPSK::new(amplitude) (symbol map only) oqpsk.rs:9-13 */
    /* Phasors whose (i, q) also depend on the symbol count or the sample index. They have no
     * LUT (modem_phasor_lut returns MODEM_ERR_UNSUPPORTED): pass the descriptor to
     * modem_tx_create as modem_tx_desc.phasor (sample-and-hold only, ntaps == 0). */
    MODEM_PHASOR_DCQPSK = 8, /* DCQPSK::new(amplitude)                 dcqpsk.rs:16-21 */
    MODEM_PHASOR_CPFSK = 10, /* CPFSK::new(bps, rates, amp, deviation) cpfsk.rs:15-25; freq =
                              * Freq::new(deviation * baud / 2, sr).sample_freq() */
    MODEM_PHASOR_MSK = 11,   /* MSK::new(amplitude, samples_per_symbol) msk.rs:13-21 */
    /* Phasors that carry a phase from symbol to symbol in f32 (update() at every symbol
     * tick): the symbol states are computed by an exact serial scan on the device, then
     * evaluated per sample; exact, but one stream scans at tens of Msymbols/s. */
    MODEM_PHASOR_DMPSK = 9,  /* DMPSK::new(bps, amplitude, phase, shift) dmpsk.rs:16-23 */
    MODEM_PHASOR_MFSK = 12,  /* MFSK::new(bps, deviation, amplitude, map) mfsk.rs:46-59;
                              * freq = deviation.sample_freq(), mfsk_map 1 = IncreaseMap */
    MODEM_PHASOR_BFSK = 13   /* BFSK::new(deviation, amplitude)        bfsk.rs:12-20; freq as MFSK */
} modem_phasor_kind;

typedef struct { uint8_t start, end; float radius, phase; } modem_ring; /* apsk.rs:60-82 */

typedef struct {
    int32_t kind;                /* modem_phasor_kind */
    uint32_t bits_per_symbol;    /* QAM/MPSK/APSK; implied for the others */
    float phase;                 /* BPSK/QPSK/QAM phase, MPSK phase_offset */
    float amplitude;
    uint32_t nrings;             /* APSK */
    const modem_ring* rings;     /* APSK */
    float freq;                  /* CPFSK: its sample frequency (cpfsk.rs:20-21); MFSK, BFSK:
                                  * the deviation's sample frequency */
    uint32_t samples_per_symbol; /* MSK: samples per symbol (even, msk.rs:14) */
    float shift;                 /* DMPSK: phase step per symbol value (dmpsk.rs:20); its
                                  * initial phase is `phase` */
    uint32_t mfsk_map;           /* MFSK: 0 = DefaultMap (2s - max), 1 = IncreaseMap (2s) */
} modem_phasor_desc;

/* Slicer description; fill it with modem_phasor_slicer() or by hand. */
typedef struct {
    int32_t kind;                /* modem_slicer_kind */
    uint32_t bits_per_symbol;
    const float* lut;            /* NEAREST: 2 * 2^bps floats (i,q), host memory */
    uint32_t bits_per_carrier;   /* QAM_AXIS */
    float inv_scale;             /* QAM_AXIS: 1 / QAM amplitude scale (qam.rs:28) */
    float max_symbol;            /* QAM_AXIS: 2^bits_per_carrier - 1 */
} modem_slicer_desc;

const char* modem_status_str(modem_status s);
int32_t modem_abi_version(void);

/* Freq::new(hz, sr).sample_freq() — freq.rs:19-26 (f32, bit-exact). */
float modem_freq_sample_freq(uint64_t hz, uint64_t sr);
/* Rates::new(br, sr).samples_per_symbol — rates.rs:12-18. br == 0 -> INVALID_ARG. */
modem_status modem_rates_sps(uint64_t br, uint64_t sr, uint64_t* sps);
/* Carrier phase of absolute sample n, bit-exact to carrier.rs:17-19 + util.rs:3-6. */
float modem_carrier_phase(float sample_freq, uint64_t n);
/* The same phase for n consecutive samples s0.. computed by the device code path the
 * kernels use (out: n floats, device pointer; asynchronous on stream). */
modem_status modem_carrier_phases(float sample_freq, uint64_t s0, size_t n, float* out,
                                  int device, void* stream);
/* Bits per symbol of a phasor (DigitalPhasor::bits_per_symbol, phasor.rs:2). */
modem_status modem_phasor_bits(const modem_phasor_desc* d, uint32_t* bps);
/* (I,Q) table of a memoryless phasor: lut[2s], lut[2s+1] = i(_, b), q(_, b) where b are
 * the bits of s MSB-first (bytes_to_bits, digital/util.rs:5-11). 2*2^bps floats. */
modem_status modem_phasor_lut(const modem_phasor_desc* d, float* lut);
/* Pick the cheapest exact slicer for a phasor: QAM_AXIS for QAM at phase 0, else NEAREST
 * (lut must then stay valid until the RX handle is created). */
modem_status modem_phasor_slicer(const modem_phasor_desc* d, const float* lut,
                                 modem_slicer_desc* out);
/* Root-raised-cosine taps (GLUE, absent from the reference): centred at (L-1)/2,
 * roll-off beta, unit energy. */
modem_status modem_rrc_taps(uint32_t ntaps, uint32_t sps, double beta, float* out);
/* The same pulse sampled at t = (i - (ntaps-1)/2 - offset) / sps, offset a finite double in samples
 * (else INVALID_ARG), normalised to unit energy; offset == 0 is modem_rrc_taps bit for bit. A TX
 * shaped with these taps is the nominal TX delayed by `offset` samples: how a stream with a
 * fractional timing offset is made. */
modem_status modem_rrc_taps_offset(uint32_t ntaps, uint32_t sps, double beta, double offset, float* out);

/* ---- TX: DigitalModulator + pulse shaping ------------------------------------------------ */
typedef struct modem_tx modem_tx;
typedef struct {
    uint32_t bits_per_symbol;    /* 1..8 */
    const float* lut;            /* 2 * 2^bps floats from modem_phasor_lut (host memory);
                                  * unused when `phasor` is set */
    uint32_t samples_per_symbol; /* Rates::samples_per_symbol, >= 1 */
    const float* taps;           /* pulse-shaping FIR (host memory) */
    uint32_t ntaps;              /* 0 = the reference's sample-and-hold (no FIR) */
    float sample_freq;           /* Freq::sample_freq() of the carrier */
    uint64_t s0;                 /* Carrier.sample at the first output sample */
    int32_t dtype;               /* modem_dtype of the output samples */
    int32_t out_mode;            /* modem_out_mode */
    uint32_t q_offset;           /* 0: Bits source. samples_per_symbol / 2: EvenOddOffset(Bits)
                                  * (data.rs:81-123, what modulate uses for oqpsk, modulate.rs:101-107):
                                  * Q changes half a symbol after I, and before the first Q tick
                                  * the phasor sees bit 0 (data.rs:84 `cur: [0, 0]`). Requires
                                  * bits_per_symbol == 2 and an even samples_per_symbol
                                  * (data.rs:91-92 asserts). With taps, the Q impulses sit at the
                                  * Q ticks (GLUE). */
    const modem_phasor_desc* phasor; /* NULL, or a DCQPSK / CPFSK / MSK phasor evaluated per
                                  * sample as DigitalModulator does (modulator.rs:85-100: the
                                  * symbol count since the stream start, and the carrier sample
                                  * index after Carrier::next); copied at create. */
} modem_tx_desc;

modem_status modem_tx_create(const modem_tx_desc* d, int device, modem_tx** out);
/* Consume `nbits` bits (one byte per bit, values 0/1 — data.rs:36) and write
 * floor((carry + nbits) / bps) * sps samples (2 values per sample for IQ modes, 1 for
 * OUT_REAL, each f32 or f16). Leftover bits (< bps) carry into the next call.
 * `cap` is in samples. */
modem_status modem_tx_process(modem_tx* h, const uint8_t* bits, size_t nbits, void* out,
                              size_t cap, size_t* produced, void* stream);
/* Several independent channels (distinct handles) in one call: the same results and handle
 * states as modem_tx_process(hs[c], bits[c], nbits[c], outs[c], caps[c], &produced[c], stream)
 * for c = 0 .. nch-1 in order. When every handle has the same matrix-core configuration
 * (sps, taps, bits per symbol, mixed I/Q output of one dtype, device) and every buffer is
 * device memory, up to 8 channels share one kernel launch. When every handle has the same
 * scanned phasor kind (DMPSK, MFSK, BFSK: a serial f32 state recurrence per stream,
 * dmpsk.rs:29-33, mfsk.rs:68-75, bfsk.rs:42-53) and every buffer is device memory (outs[c] may
 * be NULL for a channel that completes no symbol), the
 * channels' state scans run as one launch, one lane per channel, each bit for bit its single
 * call's. Otherwise the calls run one by one.
 * No reference counterpart (the reference drives one DigitalModulator per stream,
 * modulator.rs:64-101): the multi-channel form of that loop, SURVEY.md §8e. */
modem_status modem_tx_process_batch(modem_tx* const* hs, size_t nch, const uint8_t* const* bits,
                                    const size_t* nbits, void* const* outs, const size_t* caps,
                                    size_t* produced, void* stream);
/* Append ceil((ntaps-1)/sps) all-zero symbols so the FIR tail drains. */
modem_status modem_tx_flush(modem_tx* h, void* out, size_t cap, size_t* produced, void* stream);
/* Samples that the next call will start at (Carrier.sample, carrier.rs:6). */
uint64_t modem_tx_sample(const modem_tx* h);
/* The per-symbol states that the serial scan of a DMPSK / MFSK / BFSK handle left on the device in
 * its most recent modem_tx_process / modem_tx_process_batch call, copied to host memory `out`:
 * one (x, y) pair of f32 per symbol that call produced (2 * *n floats), the state after the
 * phasor's update() at that symbol's tick (dmpsk.rs:29-33, mfsk.rs:68-75, bfsk.rs:42-53):
 *   DMPSK  x = phase          y = unspecified
 *   MFSK   x = cur_coef       y = phase_offset
 *   BFSK   x = phase          y = the previous bit (0.0 or 1.0)
 * `cap` is in symbols. *n is the symbol count of that call: 0 before the first call and after a
 * call that completed no symbol. cap < *n: MODEM_ERR_CAPACITY with *n set and `out` untouched. A
 * handle whose phasor carries no scanned state: MODEM_ERR_UNSUPPORTED. Synchronises `stream` (pass
 * the stream of that call) before it returns. For tests and diagnostics: it exposes the f32
 * recurrence whose values the samples only show through sin / cos. */
modem_status modem_tx_scan_states(const modem_tx* h, float* out, size_t cap, size_t* n, void* stream);
/* How that call computed them: 1 = the handle's own scan launch (modem_tx_process, or a batch that
 * ran its calls one by one), 2 = the bank launch of modem_tx_process_batch (one lane per channel),
 * 0 = no such call yet or not a scanned phasor, -1 = h == NULL. The states are the same either way. */
int modem_tx_scan_path(const modem_tx* h);
modem_status modem_tx_destroy(modem_tx* h);

/* ---- RX: Demodulator + matched filter + decimation + slicer ----------------------------- */
typedef struct modem_rx modem_rx;
typedef struct {
    float sample_freq;           /* carrier (demodulator.rs:20) */
    uint64_t s0;                 /* Carrier.sample of the first input sample */
    const float* taps;           /* matched filter / lowpass (host memory) */
    uint32_t ntaps;              /* >= 1 */
    uint32_t decim;              /* keep every decim-th filter output; 1 = full rate */
    uint32_t decim_offset;       /* keep outputs n = k*decim + decim_offset (stream index) */
    int32_t mix;                 /* modem_mix */
    int32_t in_dtype;            /* modem_dtype of the input I/Q samples */
    int32_t out_dtype;           /* modem_dtype of the decimated I/Q output */
    modem_slicer_desc slicer;    /* decisions (kind NONE for none) */
    float phase_offset;          /* PLL::phase_offset added to every carrier phase
                                  * (demodulator.rs:50); 0 = unlocked. See modem_pll_lock. */
} modem_rx_desc;

modem_status modem_rx_create(const modem_rx_desc* d, int device, modem_rx** out);
/* Consume n complex input samples (interleaved i,q); write the decimated filter outputs
 * (interleaved i,q; may be NULL) and u8 decisions (may be NULL) for every kept instant in
 * this chunk. `cap` is in symbols. */
modem_status modem_rx_process(modem_rx* h, const void* in, size_t n, void* out_iq,
                              uint8_t* out_sym, size_t cap, size_t* produced, void* stream);
/* Several channels in one call, as modem_rx_process on each handle in order (out_iq[c] and
 * out_sym[c] may be NULL). Fused into one launch per 8 channels when every handle has the
 * same matrix-core configuration (decimation, taps, complex mix, one I/Q dtype in and out,
 * device) and every buffer is device memory. The multi-channel form of Demodulator::next
 * (demodulator.rs:44-56), SURVEY.md §8e. */
modem_status modem_rx_process_batch(modem_rx* const* hs, size_t nch, const void* const* ins, const size_t* ns,
                                    void* const* out_iq, uint8_t* const* out_sym, const size_t* caps,
                                    size_t* produced, void* stream);
/* Feed ntaps-1 zero samples (drains the matched filter). */
modem_status modem_rx_flush(modem_rx* h, void* out_iq, uint8_t* out_sym, size_t cap,
                            size_t* produced, void* stream);
uint64_t modem_rx_sample(const modem_rx* h);
modem_status modem_rx_destroy(modem_rx* h);

/* ---- One TX -> RX period over fixed device buffers ------------------------------------- */
/* A prepared step of the sample-buffer loop: modem_chain_run(c) equals
 *   modem_tx_process(tx, bits, nbits, samples, cap, &n, stream);
 *   modem_rx_process(rx, samples, n, out_iq, out_sym, out_cap, &k, stream);
 * (produced = n, produced_out = k), with the buffers checked once by modem_chain_create:
 * device memory of the handles' one device (else INVALID_ARG); the TX writes interleaved
 * complex samples (MODEM_OUT_IQ_MIXED or BASEBAND) of the RX's in_dtype. The handles stay
 * usable on their own; the plan keeps pointers to them and to the buffers (destroy it first). */
typedef struct modem_chain modem_chain;
modem_status modem_chain_create(modem_tx* tx, modem_rx* rx, const uint8_t* bits, size_t nbits,
                                void* samples, size_t cap, void* out_iq, uint8_t* out_sym,
                                size_t out_cap, modem_chain** out);
modem_status modem_chain_run(modem_chain* c, size_t* produced, size_t* produced_out, void* stream);
/* How the last modem_chain_run ran: 1 or 2 = one launch (the TX and RX of the period fused:
 * small calls with the common filters, tile geometry permitting; 2 = the form with one RX tile
 * per workgroup that hands the samples over in LDS; results identical either way), 0 = the two
 * launches, -1 = no run yet or c == NULL. MODEM_CHAIN_FUSED=0 in the environment at create time
 * forces 0. */
int modem_chain_fused(const modem_chain* c);
modem_status modem_chain_destroy(modem_chain* c);

/* A prepared step of a channel bank (independent channel streams, BASELINE
 * config 4): modem_chain_batch_run(c) equals, for every channel i < nch,
 *   modem_tx_process(txs[i], bits[i], nbits[i], samples[i], caps[i], &n[i], stream);
 *   modem_rx_process(rxs[i], samples[i], n[i], out_iq[i], out_sym[i], out_caps[i], &k[i], stream);
 * run as one TX launch and then one RX launch per `group` consecutive channels (1 <= group <= 8;
 * a group of at most 192 MiB of samples is re-read from the Infinity Cache, a larger one — C4's
 * default 8 x 32 MiB — is stored non-temporally and re-read from HBM, which measured faster
 * for it, profiles/r05_c4_policy.txt). modem_chain_batch_create
 * checks the buffers (device memory of the handles' one device) and the handles (one matrix-core
 * configuration for all TX and one for all RX handles, distinct handles, RX in_dtype = TX dtype,
 * complex mix, interleaved complex TX output) once: INVALID_ARG / UNSUPPORTED otherwise, nothing
 * created. produced / produced_out (nch entries each, may be NULL) receive n[i] and k[i].
 * With more than one group the groups alternate between `stream` and a stream of the plan's
 * own (joined to `stream` by events at the start and end of every run), so that one group's RX
 * overlaps the next group's TX; the run is asynchronous on `stream` as a whole.
 * MODEM_CHAIN_BATCH_LANES=1 in the environment at create time keeps every launch on `stream`.
 * Errors: CAPACITY (checked for every channel before any launch) leaves every handle untouched;
 * a launch error (HIP) part-way through a run leaves the groups before it advanced and the
 * rest not, so the plan is marked failed and every later run returns MODEM_ERR_HIP (destroy
 * it; its handles' streams no longer line up). The caller's stream is still joined to the
 * plan's own (best effort) so that it stays ordered after the launches already queued. */
typedef struct modem_chain_batch modem_chain_batch;
modem_status modem_chain_batch_create(modem_tx* const* txs, modem_rx* const* rxs, size_t nch, size_t group,
                                      const uint8_t* const* bits, const size_t* nbits, void* const* samples,
                                      const size_t* caps, void* const* out_iq, uint8_t* const* out_sym,
                                      const size_t* out_caps, modem_chain_batch** out);
modem_status modem_chain_batch_run(modem_chain_batch* c, size_t* produced, size_t* produced_out, void* stream);
modem_status modem_chain_batch_destroy(modem_chain_batch* c);

/* Demodulator::lock_phase (demodulator.rs:32-36): PLL::handle (pll.rs:16-22) over the n
 * complex samples x_iq (host memory; the reference uses n = 64), with the carrier phases of
 * samples s0 .. s0+n-1, starting from *phase_offset (0 for a new PLL). Control logic over a
 * few serial samples: evaluated on the host with the reference's f32 operations. */
modem_status modem_pll_lock(float sample_freq, uint64_t s0, const float* x_iq, size_t n,
                            float* phase_offset);

/* ---- FIRFilter: real-valued causal FIR over a stream (fir.rs:3-35) ---------------------- */
typedef struct modem_fir modem_fir;
modem_status modem_fir_create(const float* taps, uint32_t ntaps, int device, modem_fir** out);
/* out[i] = FIRFilter::add(in[i]) for consecutive samples (f32, same count in and out),
 * bit-identical: the reference's fold order, separate multiply and add. */
modem_status modem_fir_process(modem_fir* h, const float* in, float* out, size_t n, void* stream);
modem_status modem_fir_destroy(modem_fir* h);

/* ---- Soft-decision demapper (GLUE: the reference has no soft output) --------------------- */
/* Per-bit max-log LLRs of received points r = (re, im) — the decimated I/Q that modem_rx_process
 * writes — against a constellation lut[s] = (lut[2s], lut[2s+1]), s = 0 .. 2^bps - 1:
 *   d(s)           = (re - lut[2s])^2 + (im - lut[2s+1])^2     (the differences in f32, as the
 *                                                                NEAREST slicer forms them)
 *   llr[k*bps + j] = scale * (min_{s: bit_j(s)=1} d(s) - min_{s: bit_j(s)=0} d(s))
 * where bit j of s is (s >> (bps-1-j)) & 1: j = 0 is the MSB, the order of bytes_to_bits
 * (digital/util.rs:5-11) and of the TX's one-byte-per-bit input. A positive LLR means "bit 0 is
 * more likely"; the hard bit is llr < 0. Pass scale = 1/N0 (times a quantiser gain if wanted).
 * Output dtypes: F32; F16 (round to nearest, saturating to +-65504, never inf); I8
 * (rint(clamp(llr, -127, 127))). Input: F32 or F16 I/Q (F16 widened exactly). NaN input:
 * unspecified.
 * Two device paths with the same results up to f32 rounding: when the table is, bitwise, a product
 * grid with an even bit split (lut[2((a<<h)|b)] depends only on a, lut[2((a<<h)|b)+1] only on
 * b, h = bps/2: every QAM at phase 0) MODEM_DEMAP_AUTO evaluates the 2^h levels per axis
 * instead of the 2^bps points; MODEM_DEMAP_GENERAL forces the all-points path. */
typedef struct modem_demap modem_demap;
typedef enum { MODEM_DEMAP_AUTO = 0, MODEM_DEMAP_GENERAL = 1 } modem_demap_path_req;

/* lut: 2 * 2^bps floats from modem_phasor_lut (host memory, copied). */
modem_status modem_demap_create(const float* lut, uint32_t bits_per_symbol, int32_t in_dtype,
                                int32_t out_dtype, int32_t path, int device, modem_demap** out);
/* iq: nsym interleaved (i,q) of in_dtype; llr: nsym*bps values of out_dtype; cap in LLR values
 * (cap < nsym*bps: CAPACITY, nothing written). The handle carries no stream state: cutting a
 * buffer into several calls gives bit-identical output. scale must be finite. */
modem_status modem_demap_process(modem_demap* h, const void* iq, size_t nsym, float scale,
                                 void* llr, size_t cap, void* stream);
int modem_demap_path(const modem_demap* h);   /* 1 = axis, 0 = general, -1 = NULL */
modem_status modem_demap_destroy(modem_demap* h);

/* ---- Noncoherent detectors (GLUE: the reference's Demodulator ends at filtered I/Q) ------- */
/* Receivers for the phasors that carry state from symbol to symbol, which have no (I,Q) table and
 * so neither a slicer nor a demapper: DMPSK (the information is in phase differences) and MFSK /
 * BFSK (in tone energies). Neither needs a carrier-phase lock. Both produce, per symbol, a metric
 * c(s) for every symbol value s and from it
 *   sym[k]         = argmax_s c(s), lowest index on ties
 *   llr[k*bps + j] = scale * (max_{s: bit_j(s)=0} c(s) - max_{s: bit_j(s)=1} c(s))
 * with the demapper's bit order (bit j of s is (s >> (bps-1-j)) & 1, j = 0 the MSB), sign (a
 * positive LLR means "bit 0 is more likely"; the hard bit is llr < 0), LLR dtypes (F32; F16
 * saturating to +-65504; I8 = rint(clamp(llr, -127, 127))) and input dtypes (F32, or F16 widened
 * exactly). scale must be finite. out_sym and llr may each be NULL. NaN input: unspecified. */

/* Table of the differential detector for a DMPSK phasor (dmpsk.rs:29-33: the phase advances by
 * `s as f32 * shift` at every symbol): lut[2s], lut[2s+1] = cos(a_s), sin(a_s), a_s the f32
 * product (float)s * d->shift of dmpsk.rs:32, widened to double; cos and sin evaluated in double
 * and rounded to f32. 2 * 2^bps floats. Any other phasor kind: MODEM_ERR_UNSUPPORTED. */
modem_status modem_phasor_diff_lut(const modem_phasor_desc* d, float* lut);
/* Tone frequencies of an MFSK or BFSK phasor in radians per sample, 2^bps floats:
 *   omega[m] = carrier_sample_freq + coef(m) * d->freq      (in double from the f32 inputs,
 *                                                            rounded to f32)
 *   MFSK DefaultMap   coef(m) = 2m - (2^bps - 1)   mfsk.rs:23-27
 *   MFSK IncreaseMap  coef(m) = 2m                 mfsk.rs:31-35
 *   BFSK              coef(m) = m, bps = 1         bfsk.rs:27-29
 * Pass the carrier's Freq::sample_freq() for MODEM_OUT_IQ_MIXED streams (the phasor's tone rides
 * on the carrier, modulator.rs:45-48) and 0 for MODEM_OUT_IQ_BASEBAND streams. Any other phasor
 * kind: MODEM_ERR_UNSUPPORTED. */
modem_status modem_phasor_tones(const modem_phasor_desc* d, float carrier_sample_freq, float* omega);

/* Differential detector, at symbol rate on the decimated I/Q that modem_rx_process writes
 * (receives DMPSK, dmpsk.rs:29-43). For the received points r[k]:
 *   z[k] = r[k] * conj(r[k-1])                    (f32)
 *   c(s) = z.re * lut[2s] + z.im * lut[2s+1]
 * r[-1] is the last point of the previous call; for the first call it is prev0 (host memory, two
 * floats; NULL = (1, 0)). For a DMPSK transmitter prev0 = amplitude * (cos phase, sin phase): its
 * first symbol is already a step away from the initial phase (modulator.rs:91-93). The handle
 * carries that one point: cutting a buffer into several calls, calls with nsym == 0 included,
 * gives bit-identical output. lut: 2 * 2^bps floats (host memory, copied), from
 * modem_phasor_diff_lut or by hand. */
typedef struct modem_diff modem_diff;
modem_status modem_diff_create(const float* lut, uint32_t bits_per_symbol, const float prev0[2],
                               int32_t in_dtype, int32_t llr_dtype, int device, modem_diff** out);
/* iq: nsym interleaved (i,q) of in_dtype; out_sym: nsym bytes; llr: nsym*bps values of llr_dtype;
 * cap in symbols (cap < nsym: CAPACITY, nothing written, the state unchanged). */
modem_status modem_diff_process(modem_diff* h, const void* iq, size_t nsym, float scale,
                                uint8_t* out_sym, void* llr, size_t cap, void* stream);
modem_status modem_diff_destroy(modem_diff* h);

/* Tone-bank energy detector, at sample rate directly on the complex samples that modem_tx_process
 * writes (receives MFSK, mfsk.rs:60-75, and BFSK, bfsk.rs:23-55). Symbol k covers the stream
 * samples k*sps .. k*sps + sps-1, counted from the handle's first input sample — the samples the
 * modulator emits while symbol k is current (modulator.rs:85-100):
 *   S[k,m] = sum_{i<sps} x[k*sps+i] * e^{-j*omega[m]*i}        (f32 accumulation, i ascending)
 *   c(m)   = E[k,m] = S.re^2 + S.im^2
 *   energy[k*2^bps + m] = E[k,m]                                (f32, may be NULL)
 * The phase index i is relative to the symbol: a constant phase drops out of |S|^2, so the detector
 * needs no carrier sample counter, and the phasor's f32 `s as f32` (mfsk.rs:61) does not enter.
 * omega: 2^bps finite floats (host memory), from modem_phasor_tones or by hand; the twiddles are
 * tabulated at create time (cos and sin of the double product omega[m] * i, rounded to f32).
 * samples_per_symbol * 2^bps > 65536 (a 512 KiB table): MODEM_ERR_UNSUPPORTED.
 * Streaming: the handle carries the < sps samples after the last whole symbol;
 * *produced = floor((carried + n) / sps); cuts at any sample positions, n == 0 included, give
 * output bit-identical to one call. cap in symbols (*produced > cap: CAPACITY, nothing written,
 * the state unchanged). */
typedef struct modem_fsk modem_fsk;
modem_status modem_fsk_create(const float* omega, uint32_t bits_per_symbol, uint32_t samples_per_symbol,
                              int32_t in_dtype, int32_t llr_dtype, int device, modem_fsk** out);
modem_status modem_fsk_process(modem_fsk* h, const void* in, size_t n, float scale, uint8_t* out_sym,
                               void* llr, float* energy, size_t cap, size_t* produced, void* stream);
modem_status modem_fsk_destroy(modem_fsk* h);

/* ---- Channel model (GLUE: the reference has no channel) ------------------------------------ */
/* The stage between modem_tx_process and modem_rx_process: gain, an NCO frequency / phase offset
 * and seeded additive white Gaussian noise on a buffer of interleaved complex samples. For the
 * absolute sample index n (the handle's s0 plus the position in the stream) and the input x[n]:
 *
 *   y[n] = gain * x[n] * e^{j*theta[n]} + sqrt(n0) * w[n]
 *
 * NCO, exact for any n:
 *   theta[n] = 2*pi * ((phase0 + step*n) mod 2^64) / 2^64
 * phase0 and step are uint64_t, fixed at create time from the doubles `phase` (radians) and `cfo`
 * (radians per sample; both may be negative): each value v becomes frac(v / (2*pi)) * 2^64, rounded
 * to nearest and wrapped mod 2^64 (evaluated with enough bits of pi for every finite double).
 * modem_chan_nco reads the two integers back; they, not the doubles, define the rotation, which
 * therefore neither degrades at large n nor depends on where the calls cut the stream.
 *
 * Noise, counter-based on n, with mix() the splitmix64 finaliser of modem_prng_bits
 * (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31),
 * GOLDEN = 0x9E3779B97F4A7C15 and uint64 wrap-around arithmetic:
 *   k     = mix(seed + GOLDEN)                    the first word modem_prng_bits emits for `seed`
 *   word  = mix(k + (n+1)*GOLDEN)
 *   u1    = ((word >> 40) + 1) * 2^-24            in (0, 1], exact in f32
 *   u2    = ((word & 0xffffffff) >> 8) * 2^-24    in [0, 1), exact in f32
 *   w[n]  = sqrt(-ln u1) * (cos 2*pi*u2, sin 2*pi*u2)
 * E|w|^2 = 1: n0 is the complex noise variance (n0/2 per rail), the N0 of the scale = 1/N0 that
 * modem_demap_process, modem_diff_process and modem_fsk_process document. For a unit-energy matched
 * filter and symbols of mean energy A^2 carrying bps bits, Eb/N0 = A^2 / (bps * n0).
 * Limit: |w| <= sqrt(24 ln 2) ~ 4.08 (u1 >= 2^-24), so the tail is cut at about 5.8 per-rail sigma.
 *
 * Arithmetic: everything after the integer parts is f32 (the angle from the top 32 bits of the
 * phase). F16 input is widened exactly; F16 output is rounded to nearest even, as the TX stores it
 * (beyond the f16 range: unspecified). NaN input: unspecified output. With n0 == 0 no noise is
 * evaluated; with step == 0 and phase0 == 0 no rotation; with gain == 1 as well the output equals
 * the input as values (a -0 may become +0).
 *
 * Streaming: the handle's only stream state is the sample counter; cutting a buffer into several
 * calls at any positions, calls with n == 0 included, gives bit-identical output. */
typedef struct modem_chan modem_chan;
/* gain, phase, cfo finite; n0 finite and >= 0; in_dtype, out_dtype F32 or F16 (any of the four
 * pairs), else INVALID_ARG. The handle owns no device memory, so creating it touches no device:
 * device < 0 is NO_DEVICE here, any other ordinal is checked by the first modem_chan_process. */
modem_status modem_chan_create(double gain, double phase, double cfo, double n0, uint64_t seed, uint64_t s0,
                               int32_t in_dtype, int32_t out_dtype, int device, modem_chan** out);
/* in: n interleaved (i,q) of in_dtype; out: n of out_dtype; cap in samples (cap < n: CAPACITY,
 * nothing written, the state unchanged); n == 0 is valid. out == in (in place) is allowed when the
 * dtypes are equal; any other overlap of the two byte ranges, or a stream that would pass sample
 * 2^64: INVALID_ARG. Device or host pointers, as modem_demap_process. */
modem_status modem_chan_process(modem_chan* h, const void* in, size_t n, void* out, size_t cap, void* stream);
/* A new noise variance from the next call on (Eb/N0 sweeps over one stream). */
modem_status modem_chan_set_n0(modem_chan* h, double n0);
/* The NCO integers (either pointer may be NULL). */
modem_status modem_chan_nco(const modem_chan* h, uint64_t* step, uint64_t* phase0);
/* The n of the next input sample (0 for NULL). */
uint64_t modem_chan_sample(const modem_chan* h);
modem_status modem_chan_destroy(modem_chan* h);

/* Error counter for one-byte-per-bit or one-byte-per-symbol decisions:
 *   counts[0] += #{i < n : a[i] != b[i]}          counts[1] += sum_{i<n} popcount(a[i] ^ b[i])
 * counts points to two uint64_t that are accumulated into, never cleared: the caller zeroes them.
 * a, b and counts are all device pointers (asynchronous on `stream`; counts 8-byte aligned) or all
 * host pointers (synchronous); a mix: INVALID_ARG. */
modem_status modem_count_errors(const uint8_t* a, const uint8_t* b, size_t n, uint64_t* counts, int device,
                                void* stream);

/* ---- Carrier synchronizer (GLUE: the reference has none) ----------------------------------- */
/* A non-data-aided feedforward carrier synchronizer at symbol rate, on the decimated I/Q that
 * modem_rx_process writes and in front of modem_demap_process or a slicer: block M-th-power
 * (Viterbi & Viterbi) phase estimates, unwrapped across blocks, applied as a piecewise-linear
 * derotation. It removes what modem_chan_create's `phase` and `cfo` put in.
 *
 * Parameters: power = M in {2, 4, 8}, the constellation's rotational symmetry (lm = log2 M);
 * block = B, symbols per block, a power of two in 64 .. 4096 (lb = log2 B); norm, a finite double
 * > 0 applied (as f32) before the power, 1 / rms of the constellation; ref_phase, the argument of
 * sum_s (norm * lut[s])^M over the constellation (pi for square QAM), and phase0, where the tracker
 * starts, finite doubles in radians turned into uint64 fractions of a turn exactly as
 * modem_chan_create turns `phase` into phase0 (`ref`, `phase0` below); flags: MODEM_SYNC_FLAT.
 *
 * For the stream's symbols r[k], k counted from the handle's first input symbol (after a flush:
 * from the first symbol after it), block b covers k = b*B .. b*B + B-1.
 *
 * 1. Per block, in f32:  z[k] = (norm * r[k])^M by lm complex squarings ((a, b) -> (a*a - b*b,
 *    2*a*b)), |z[k]| = (|norm * r[k]|^2)^(M/2), P_b = sum z[k], S_b = sum |z[k]|. The summation
 *    order depends on the offset i = k - b*B alone, never on where calls cut the stream: the terms
 *    with the same i mod 256 are added with i ascending, starting from 0 (at most 16 terms); for
 *    each l = i mod 64 the four sums of i mod 256 = l, l+64, l+128, l+192 are joined as
 *    (t0 + t1) + (t2 + t3); the 64 results are joined by a balanced tree that pairs l with
 *    l xor 32, then xor 16, 8, 4, 2, 1.
 * 2. q_b = |P_b| / S_b, 0 when S_b is 0 or anything is not finite.
 *    Phi_b = ((uint64_t)turn(P_b.im, P_b.re) << 32) - ref, where turn(y, x) is atan2(y, x) as a
 *    32-bit fraction of a turn, within 2^-22 turns of the exact angle; turn(0, 0) and non-finite
 *    input give 0.
 * 3. Unwrap, exact in uint64 / int64 ring arithmetic (sext64: the value read as int64; >> on it
 *    arithmetic):
 *      theta_b = theta_{b-1} + (sext64(Phi_b - Phi_{b-1}) >> lm)
 *      theta_{-1} = phase0,  Phi_{-1} = M * phase0 mod 2^64
 *    so theta_0 is the branch of Phi_0 / M nearest phase0. The M-fold ambiguity is inherent: the
 *    estimator cannot tell a carrier phase from one a multiple of 1/M turn away, so the output is
 *    the constellation up to the rotation that phase0 selects, and a block whose estimate is off by
 *    more than 1/(2M) turn moves every later block by 1/M turn (a slip). Tracking range: the phase
 *    may advance by less than 1/(2M) turn per block, |cfo per symbol| < pi / (M * B) radians.
 * 4. Apply:  d_b = sext64(theta_b - theta_{b-1}), d_0 = 0 for the stream's first block;
 *    s_b = d_b >> (lb + 1), 0 under MODEM_SYNC_FLAT; for the offset i in block b
 *      ph = theta_b + s_b * (2*i - B + 1) mod 2^64         (theta_b at the block's centre)
 *      out[k] = r[k] * e^{-j*2*pi*ph / 2^64}
 *    from the top 32 bits of ph, in f32. F16 input is widened exactly, F16 output rounded to
 *    nearest even.
 * 5. Streaming: the handle carries, on the device, the < B symbols after the last whole block and
 *    theta, Phi, d of the last block. A call emits floor((carried + n) / B) blocks; any cut of a
 *    stream into calls, nsym == 0 included, gives bit-identical out, theta and quality.
 *    modem_sync_flush emits the carried symbols rotated on the last block's line extended
 *    (i -> i + B), or by phase0 (theta = phase0, s = 0) when no block was ever completed; it writes
 *    no estimates, and the handle is at a block boundary afterwards (theta, Phi and d stay). */
#define MODEM_SYNC_FLAT 1u        /* one phase per block (s_b = 0) instead of the line through the centres */
typedef struct modem_sync modem_sync;
/* Bad power, block, norm, phases, flags, dtypes (F32 or F16, any of the four pairs) or a NULL out:
 * INVALID_ARG, before any device is looked at. The handle owns device memory: a bad ordinal is
 * NO_DEVICE here. */
modem_status modem_sync_create(uint32_t power, uint32_t block, double norm, double ref_phase, double phase0,
                               uint32_t flags, int32_t in_dtype, int32_t out_dtype, int device, modem_sync** out);
/* iq: nsym interleaved (i,q) of in_dtype; out: *produced = *blocks * B symbols of out_dtype, cap in
 * symbols; theta (uint64_t) and quality (float), one per block, either may be NULL, est_cap in
 * blocks. cap or est_cap too small: CAPACITY, nothing written, the state unchanged. The output lags
 * the input by the carried symbols, so there is no in-place form: overlapping byte ranges of iq
 * and out are INVALID_ARG. Device or host pointers, as modem_demap_process. */
modem_status modem_sync_process(modem_sync* h, const void* iq, size_t nsym, void* out, size_t cap, uint64_t* theta,
                                float* quality, size_t est_cap, size_t* produced, size_t* blocks, void* stream);
/* The carried symbols (*produced < B of them); cap in symbols, too small: CAPACITY as above. */
modem_status modem_sync_flush(modem_sync* h, void* out, size_t cap, size_t* produced, void* stream);
/* The number of input symbols taken so far (0 for NULL). */
uint64_t modem_sync_symbol(const modem_sync* h);
modem_status modem_sync_destroy(modem_sync* h);

/* ---- Symbol timing synchronizer (GLUE: the reference has none) ------------------------------ */
/* A non-data-aided feedforward symbol timing synchronizer at sample rate, on the I/Q that
 * modem_rx_process writes with decim = 1 (the matched-filter output at N samples per symbol) and in
 * front of modem_sync_process: block square-law (Oerder & Meyr) delay estimates from the
 * symbol-rate line of |x|^2, unwrapped across blocks, applied as a piecewise-linear delay through
 * a 4-tap cubic Lagrange interpolator. It emits one point per symbol, at the centre of the eye.
 * The estimate is blind to carrier phase and frequency offset. The chain is
 * rx(decim = 1) -> timing -> carrier synchronizer -> demapper.
 *
 * Parameters: sps = N, samples per symbol, 4 or 8 (ln = log2 N); block = B, symbols per block, a
 * power of two in 32 .. 4096 (lb = log2 B); span, in symbols, 1 .. 16: the tracked delay is kept
 * within +-span symbols; tau0, a finite double with |tau0| <= span, in symbols, where the tracker
 * starts: D_{-1} = rint(tau0 * 2^32); flags: MODEM_TIMING_FLAT.
 *
 * The input is the stream x[n], n counted from the handle's first input sample (after a flush:
 * from the first sample after it), x[n] = 0 for n < 0. Block b covers the symbols k = b*B ..
 * b*B + B-1, that is the samples b*B*N .. (b+1)*B*N - 1. Delays are int64 in units of 2^-32 symbol.
 *
 * 1. Per block, in f32:  E_p = sum_{k in block} |x[k*N + p]|^2 for p = 0 .. N-1, each term
 *    fma(re, re, im*im). The summation order depends on the sample's offset u = n - b*B*N alone,
 *    never on where calls cut the stream: the terms with the same u mod 512 are added with u
 *    ascending, starting from 0 (at most 64 terms); for each v = u mod 128 the four sums of
 *    u mod 512 = v, v+128, v+256, v+384 are joined as (t0 + t1) + (t2 + t3); the 128 / N results
 *    of one p = v mod N are joined by a balanced tree over l = v / 2 that pairs l with l xor 32,
 *    then xor 16, 8, 4 (and 2 when N = 4). S_b = (E0 + E1) + (E2 + E3), for N = 8 that plus
 *    ((E4 + E5) + (E6 + E7)). The symbol-rate line X_b = sum_p E_p e^{-j 2 pi p / N}:
 *      N = 4:  re = E0 - E2,  im = E3 - E1
 *      N = 8:  h = (float)sqrt(0.5), d_p = E_p - E_{p+4}:
 *              re = d0 + h*(d1 - d3),  im = -(d2 + h*(d1 + d3))
 *    every operation rounded on its own (no contraction).
 * 2. q_b = |X_b| / S_b, 0 when S_b is 0 or anything is not finite.
 *    Phi_b = (0 - turn32(X_b.im, X_b.re)) mod 2^32, turn32 the 32-bit angle of the carrier
 *    synchronizer (within 2^-22 turns; 0 for (0, 0) and non-finite input). Phi_b / 2^32 is the
 *    fraction of a symbol by which the centre of the eye lags the grid instants k*N.
 * 3. Unwrap, exact in int64 (sext32: the low 32 bits read as int32):
 *      D_b = D_{b-1} + sext32(Phi_b - low32(D_{b-1}))
 *    so D_b is the branch of Phi_b nearest D_{b-1}, and after the first block a prefix sum of
 *    sext32(Phi_b - Phi_{b-1}). Tracking range: the delay may move by less than half a symbol per
 *    block. tau[b] = D_b.
 * 4. Apply:  s_b = (D_b - D_{b-1}) >> (lb + 1) (arithmetic), 0 for the stream's first block and
 *    under MODEM_TIMING_FLAT; for the offset i in block b
 *      e  = clamp(D_b + s_b * (2*i - B + 1), -span * 2^32, +span * 2^32)
 *      Q  = N * ((i - span) * 2^32 + e)        Q32.32 samples relative to sample b*B*N
 *      m  = Q >> 32 (floor),  mu = ((Q & 0xffffffff) >> 8) * 2^-24   (exact in f32)
 *      out[b*B + i] = sum_{j=-1..2} c_j(mu) * x[b*B*N + m + j]
 *    in f32, each component as ((c_-1 * x_-1, then fma(c_0, x_0, .), fma(c_1, x_1, .),
 *    fma(c_2, x_2, .)), with a = mu + 1, b = mu - 1, d = mu - 2, k6 = (float)(1.0 / 6.0):
 *      c_-1 = (-((mu*b)*d)) * k6     c_0 = ((a*b)*d) * 0.5
 *      c_1  = (-((a*mu)*d)) * 0.5    c_2 = ((a*mu)*b) * k6
 *    so mu = 0 gives exactly (-0, 1, 0, -0) and out = x[b*B*N + m] bit for bit (finite taps). F16
 *    input is widened exactly, F16 output rounded to nearest even.
 *    Output symbol k is the input interpolated at the centre of the eye of grid symbol k - span:
 *    the fixed lag of `span` symbols is what lets block b be emitted the moment its last sample
 *    arrives. The clamp keeps every tap inside the samples b*B*N - 2*span*N - 1 .. (b+1)*B*N - 1;
 *    a delay outside +-span gives clamped positions: specified and memory-safe, not right. The
 *    first `span` outputs of a stream straddle the zeros before it. Which output is a frame's
 *    first symbol (integer-symbol alignment) stays with the caller.
 * 5. Streaming: the handle carries, on the device, the 2*span*N + 1 samples before the current
 *    block, the samples of the incomplete block, and D, Phi, D - D_prev of the last block. A call
 *    emits floor((carried + n) / (B*N)) blocks; any cut of a stream into calls, n == 0 included,
 *    gives bit-identical out, tau and quality. modem_timing_flush emits floor(carried / N) symbols
 *    on the last block's line extended (i -> i + B in e, i in Q), or at D_{-1} with s = 0 when no
 *    block was ever completed; samples past the end read as zero and the < N trailing samples are
 *    dropped. It writes no estimates; afterwards the handle is at a block boundary with an all-zero
 *    history, and D, Phi and D - D_prev stay. */
#define MODEM_TIMING_FLAT 1u      /* one delay per block (s_b = 0) instead of the line through the centres */
typedef struct modem_timing modem_timing;
/* Bad sps, block, span, tau0, flags, dtypes (F32 or F16, any of the four pairs) or a NULL out:
 * INVALID_ARG, before any device is looked at. The handle owns device memory: a bad ordinal is
 * NO_DEVICE here. */
modem_status modem_timing_create(uint32_t sps, uint32_t block, uint32_t span, double tau0, uint32_t flags,
                                 int32_t in_dtype, int32_t out_dtype, int device, modem_timing** out);
/* in: n interleaved (i,q) samples of in_dtype; out: *produced = *blocks * B symbols of out_dtype,
 * cap in symbols; tau (int64_t) and quality (float), one per block, either may be NULL, est_cap in
 * blocks. cap or est_cap too small: CAPACITY, nothing written, the state unchanged. An output
 * symbol gathers samples around its position, so there is no in-place form: overlapping byte ranges
 * of in and out are INVALID_ARG. Device or host pointers, as modem_sync_process. */
modem_status modem_timing_process(modem_timing* h, const void* in, size_t n, void* out, size_t cap, int64_t* tau,
                                  float* quality, size_t est_cap, size_t* produced, size_t* blocks, void* stream);
/* The symbols of the incomplete block (*produced < B of them); cap in symbols, too small: CAPACITY as above. */
modem_status modem_timing_flush(modem_timing* h, void* out, size_t cap, size_t* produced, void* stream);
/* The number of input samples taken so far (0 for NULL). */
uint64_t modem_timing_sample(const modem_timing* h);
modem_status modem_timing_destroy(modem_timing* h);

/* ---- Frame synchronizer (GLUE: the reference has none) -------------------------------------- */
/* A data-aided frame synchronizer at symbol rate, on the symbols that modem_sync_process writes and
 * in front of modem_demap_process or a slicer: a known unique word (UW) in front of each frame is
 * correlated against the stream, the peaks of the normalised correlation are the frame starts, and
 * the angle of each peak is the rotation the carrier synchronizer left (its M-fold ambiguity).
 * modem_frame_gather cuts the frames out and takes that rotation off. The chain is
 * rx -> [timing ->] carrier synchronizer -> frame synchronizer -> gather -> demapper, and needs no
 * knowledge of the channel.
 *
 * Parameters: u[0..L-1], the unique word, interleaved f32 (re, im), 8 <= L <= 256, all values
 * finite, Eu = sum |u[j]|^2 > 0 (summed in double, j ascending); guard = W, the half-width of the
 * peak window, 1 <= W <= 256; threshold = thr, a finite double in (0, 1]; in_dtype F32 or F16
 * (widened exactly). t2 = (float)(thr * thr * Eu) and the f32 (float)Eu are formed once at create.
 *
 * r[k] are the stream's symbols, k counted from the handle's first input symbol and never reset;
 * modem_frame_symbol returns the number of symbols taken so far.
 *
 * 1. Correlation and energy, in f32, for every k whose L symbols exist (inside the current window,
 *    step 5):  c[k] = sum_j r[k+j] * conj(u[j]),  e[k] = sum_j |r[k+j]|^2. The summation order
 *    depends on j alone: four accumulators (cr, ci, e), indexed by j mod 4, start at 0 and take
 *    their terms with j ascending, term j as
 *      cr = fma(r.re, u.re, cr); cr = fma(r.im, u.im, cr);
 *      ci = fma(r.im, u.re, ci); ci = fma(-r.re, u.im, ci);
 *      e  = fma(r.re, r.re, e);  e  = fma(r.im, r.im, e);
 *    and are joined as (a0 + a1) + (a2 + a3).  m[k] = fma(c.re, c.re, c.im * c.im).
 * 2. Candidates: pass[k] iff m[k] and e[k] are finite, m[k] > 0 and m[k] >= t2 * e[k] (the product
 *    rounded to f32): the normalised correlation |c| / sqrt(e Eu) >= thr, invariant to gain and to
 *    any constant phase.
 * 3. Peak picking: k is a hit iff pass[k], m[k] > m[k'] for every existing k' in k-W .. k-1 and
 *    m[k] >= m[k'] for every existing k' in k+1 .. k+W. Positions before the window's first symbol,
 *    and positions without all L symbols at a flush, do not exist and impose no condition; a
 *    non-finite m[k'] imposes none either. So among equal maxima the earliest wins, and two hits
 *    are always more than W apart.
 * 4. Per hit, in ascending k: pos (uint64_t) = k of the UW's first symbol; phi (uint32_t) =
 *    turn(c.im, c.re), the 32-bit turn fraction of the carrier synchronizer (within 2^-22 turns);
 *    metric (float) = sqrt(m / (e * (float)Eu)), division and square root correctly rounded.
 *    *count (uint64_t) = the number of hits decided in this call, never capped; only the first
 *    min(*count, cap) hits are stored and nothing past them is written, so a small cap loses hits
 *    but refuses nothing and changes no state differently.
 * 5. Streaming: position k is decided once r up to k + W + L - 1 is known. The handle carries the
 *    last 2W + L - 1 symbols on the device, in two slots: a call reads one and writes the other.
 *    Any cut of a stream into calls, nsym == 0 included, yields the same concatenated hits.
 *    modem_frame_flush decides the remaining positions that have all L symbols and drops the
 *    carry: the next symbol starts a fresh window (no position before it exists), the counter k
 *    goes on.
 * 6. Limits: the correlation is coherent over L symbols, so a residual frequency offset must
 *    satisfy |cfo per symbol| * L << 1: the stage belongs after the carrier synchronizer. The
 *    rotation is meaningful only if the UW is not mapped onto itself by a rotation of 1/M turn,
 *    which a nonzero sequence never is. */
typedef struct modem_frame modem_frame;
/* Bad len, guard, threshold, dtype, a non-finite or all-zero UW, a NULL uw or out: INVALID_ARG,
 * before any device is looked at. The handle owns device memory: a bad ordinal is NO_DEVICE here. */
modem_status modem_frame_create(const float* uw, uint32_t len, uint32_t guard, double threshold, int32_t in_dtype,
                                int device, modem_frame** out);
/* iq: nsym interleaved (i,q) of in_dtype; pos, phi, metric: cap entries each, phi and metric may be
 * NULL; a NULL pos or count is INVALID_ARG. Device or host pointers, as modem_demap_process (host
 * outputs make the call synchronous). */
modem_status modem_frame_process(modem_frame* h, const void* iq, size_t nsym, uint64_t* pos, uint32_t* phi,
                                 float* metric, size_t cap, uint64_t* count, void* stream);
modem_status modem_frame_flush(modem_frame* h, uint64_t* pos, uint32_t* phi, float* metric, size_t cap,
                               uint64_t* count, void* stream);
/* The number of input symbols taken so far (0 for NULL). */
uint64_t modem_frame_symbol(const modem_frame* h);
modem_status modem_frame_destroy(modem_frame* h);
/* Hits into frames the demapper can take; stateless. iq: nsym symbols of in_dtype, iq[0] being
 * stream symbol `base`; pos, phi: cap entries as modem_frame_process wrote them, *count its count
 * (all three read on the device, no read-back; phi NULL: no rotation); out: cap rows of len symbols
 * of out_dtype; ok: cap bytes. power = M in {1, 2, 4, 8}, lm = log2 M; rot_f = 0 for M = 1, else
 *   rot_f = ((uint32_t)(phi_f + (1u << (31 - lm)))) >> (32 - lm)
 * the multiple of 1/M turn nearest phi_f, wrapping. For each row f < cap: if f < min(*count, cap)
 * and the symbols pos_f + skip .. pos_f + skip + len - 1 all lie in [base, base + nsym), then
 *   out[f][i] = r[pos_f - base + skip + i] * e^{-j 2 pi rot_f / M}   and ok[f] = 1,
 * else the row is all zeros and ok[f] = 0. A rotation by a multiple of a quarter turn is done by
 * swaps and sign changes (exact); the odd eighths of M = 8 multiply in f32 by (c, s) =
 * cos, sin(2 pi rot_f / 8) as the channel model forms them: (fma(im, s, re * c), fma(-re, s, im * c)).
 * F16 input is widened exactly, F16 output rounded to nearest even. Bad power, dtypes, len == 0 or a
 * NULL count (or, with cap > 0, pos, out or ok): INVALID_ARG, before any device is looked at. */
modem_status modem_frame_gather(const void* iq, size_t nsym, uint64_t base, const uint64_t* pos, const uint32_t* phi,
                                const uint64_t* count, size_t cap, uint32_t skip, uint32_t len, uint32_t power,
                                int32_t in_dtype, int32_t out_dtype, void* out, uint8_t* ok, int device, void* stream);

/* ---- Convolutional code (GLUE: the reference has none) -------------------------------------- */
/* A rate-1/n convolutional code: a stateless encoder in front of modem_tx_process and a batched
 * soft-decision Viterbi decoder behind modem_demap_process, on the frames that modem_frame_gather
 * cuts out. Frames are independent: each starts in state 0 and, with MODEM_CONV_TAIL, ends there.
 * The chain is bits -> encode -> tx ... rx -> [timing ->] carrier synchronizer -> frame
 * synchronizer -> gather -> demapper -> viterbi. Every metric is an integer, so the decoder's
 * output is specified bit for bit.
 *
 * Parameters: the constraint length K, 3 <= K <= 9; n in {2, 3} generator polynomials g[j],
 * 0 < g[j] < 2^K; S = 2^(K-1) states; flags: MODEM_CONV_TAIL. With the tail, K-1 zero bits follow
 * the nbits information bits of a frame and T = nbits + K - 1 steps; without, T = nbits. A frame is
 * n * T coded bits.
 *
 * 1. Encoder step t, with input bit b (0 in the tail) and state s (0 at the start of a frame):
 *      reg = (b << (K-1)) | s;   coded bit j = parity(reg & g[j]), stored at index t*n + j;
 *      the next state is reg >> 1.
 *    The top bit of g taps the current bit, as in the usual octal notation: the customary K = 7
 *    pair is (0171, 0133).
 * 2. Decoder input: llr is rows of at least n * T values of in_dtype (F32, F16 or I8), row stride
 *    `stride` in elements; a positive value means "bit 0", the demapper's sign. Each value is
 *    quantised to an integer q before use:
 *      I8:        q = max(v, -127)
 *      F32, F16:  q = (int) rintf(fminf(fmaxf(v * qscale, -127.f), 127.f))
 *    F16 widened exactly, the product one f32 multiply, ties to even; qscale finite and positive.
 *    A NaN is unspecified (and memory-safe). q = 0 is an erasure: a caller depunctures by inserting
 *    zeros (modem_rm_rx below does).
 * 3. Path metrics are int32 correlations, maximised: pm[0] = 0 at the start of a frame, every
 *    other state -2^30. State s' at step t+1 has the input bit b = s' >> (K-2) and the two
 *    predecessors p_x = ((s' << 1) & (S-1)) | x, x in {0, 1};
 *      m_x = pm[p_x] + sum_j (1 - 2 c_j) q[t*n + j],  c_j coded bit j of reg = (b << (K-1)) | p_x.
 *    The survivor is x = 1 iff m_1 > m_0 (ties keep x = 0); dec[t][s'] = x, pm'[s'] = m_x.
 *    n * 127 * T < 2^29 under the length limit below: nothing overflows, and the start value never
 *    wins.
 * 4. Traceback: the end state is 0 with the tail, else the state of the largest final metric, the
 *    lowest index among equals. Walking back from step T-1: bit_t = s' >> (K-2), the previous state
 *    is p_x with x = dec[t][s']. The first nbits bits go to `out`, one byte per bit, rows of stride
 *    out_stride; nothing is written past nbits in a row. metric[f] (int32, may be NULL) is the end
 *    state's final metric.
 * 5. ok may be NULL; otherwise nframes bytes as modem_frame_gather writes them: a row with
 *    ok[f] == 0 is not decoded, its nbits output bytes and its metric are 0. Nothing is read back.
 * 6. Limits: this version keeps the decision bits of a frame group in LDS, 32 KiB of them:
 *    T <= 4096 for S <= 64, 2048 for S = 128, 1024 for S = 256. Longer frames, and nbits == 0, are
 *    INVALID_ARG. Streaming and sliding-window decoding of an unterminated stream are out of scope.
 *
 * Every buffer (bits, out, llr, ok, metric) is device memory of the entry's device; anything else
 * is INVALID_ARG. The calls are asynchronous on `stream`. */
#define MODEM_CONV_TAIL 1u        /* K-1 zero bits end each frame in state 0 */
/* bits: nframes rows of nbits bytes, row stride in_stride >= nbits, only bit 0 of a byte is used;
 * out: rows of n * T bytes (the TX's one-byte-per-bit input), row stride out_stride >= n * T; bytes
 * past n * T in a row are not written. Bad K, n, polynomial, flags, nbits == 0, a stride too small
 * or (with nframes > 0) a NULL pointer: INVALID_ARG, before any device is looked at; then a bad
 * ordinal is NO_DEVICE; nframes == 0 succeeds and writes nothing. */
modem_status modem_conv_encode(uint32_t K, const uint32_t* polys, uint32_t n, uint32_t flags, const uint8_t* bits,
                               size_t nframes, size_t nbits, size_t in_stride, uint8_t* out, size_t out_stride, int device,
                               void* stream);
typedef struct modem_viterbi modem_viterbi;
/* Bad K, n, polynomial, flags, dtype or a NULL polys or out: INVALID_ARG, before any device is
 * looked at. The handle holds the code's branch table on the device and no stream state: a bad
 * ordinal is NO_DEVICE here. */
modem_status modem_viterbi_create(uint32_t K, const uint32_t* polys, uint32_t n, uint32_t flags, int32_t in_dtype, int device,
                                  modem_viterbi** out);
/* A NULL handle, nbits == 0 or a frame over the limit, stride < n * T, out_stride < nbits, a qscale
 * that is not finite and positive (checked for I8 too, where it is unused), or (with nframes > 0) a
 * NULL llr or out: INVALID_ARG, before any device is looked at, and nothing is written.
 * nframes == 0 succeeds and writes nothing. */
modem_status modem_viterbi_process(modem_viterbi* h, const void* llr, size_t stride, size_t nframes, size_t nbits, float qscale,
                                   const uint8_t* ok, uint8_t* out, size_t out_stride, int32_t* metric, void* stream);
modem_status modem_viterbi_destroy(modem_viterbi* h);

/* ---- Rate matching and frame check (GLUE: the reference has none) ---------------------------- */
/* What a coded frame needs around the convolutional code: puncturing to a higher rate, a block
 * interleaver that spreads the bursts the receive chain makes, and a CRC that says whether a frame
 * decoded right. The chain is
 *   bits -> crc attach -> conv encode -> rm tx -> tx ... rx -> ... -> gather -> demapper
 *        -> rm rx -> viterbi(ok) -> crc check(ok) -> ok'
 * Everything is an integer rule on independent frames, so every output value is specified exactly.
 * The entries are stateless: the pattern and the CRC's parameters are passed by value with each
 * call (pattern is host memory, read before the call returns); nothing is kept on the device.
 *
 * 1. Puncturing. pattern[0..P-1], bytes that are 0 or 1, 1 <= P <= 64, weight w = sum pattern >= 1.
 *    A frame has Nm mother indices, 1 <= Nm <= 16384 (the n * T of modem_conv_encode's row). Index
 *    m, 0 <= m < Nm, is kept iff pattern[m mod P] == 1, and a kept m has the rank
 *      j = (m / P) * w + #{i < m mod P : pattern[i] == 1}.
 *    E = #{kept m < Nm}; a pattern with E == 0 for the Nm of the call is INVALID_ARG. For the K = 7
 *    pair (0171, 0133), coded bit t*n + j: rate 2/3 is (1,1,1,0), rate 3/4 is (1,1,1,0,0,1).
 * 2. Interleaving, over the E kept values: cols = C, 1 <= C <= 256; rows = ceil(E / C);
 *    cl = E - (rows - 1) * C (1 .. C, the cells of the last row). Input j sits at r = j / C,
 *    c = j mod C; the block is written by rows and read by columns, the absent cells of the last
 *    row skipped:
 *      pi(j) = c * rows + r - max(0, c - cl),
 *    a bijection on 0 .. E-1; C = 1 is the identity. Mother index m is transmitted at position
 *    pi(rank(m)).
 * 3. modem_rm_tx: bits is nframes rows of Nm bytes, row stride in_stride >= Nm; out is rows of E
 *    bytes, row stride out_stride >= E: out[f][pi(rank(m))] = bits[f][m] & 1 for every kept m.
 *    Nothing is written past E in a row.
 * 4. modem_rm_rx: llr is rows of E values of dtype (F32, F16 or I8), out rows of Nm values of the
 *    same dtype, strides in elements: out[f][m] = llr[f][pi(rank(m))] for a kept m, moved as bits
 *    with no arithmetic (a NaN payload, a -0 and a -128 arrive unchanged); a punctured m gets the
 *    dtype's +0 (all bits zero), the decoder's erasure. Nothing is written past Nm in a row. ok may
 *    be NULL; otherwise nframes bytes of device memory, accepted so that the chain's calls look
 *    alike, and ignored: every row is moved (the decoder behind it skips the rows with ok == 0).
 * 5. The CRC: width W in {8, 16, 24, 32}; poly (the top bit x^W implicit), init and xorout below
 *    2^W. No reflection: the message is the row's bytes in order, first byte first, bit 0 of each
 *    byte. One step per message bit b:
 *      fb = (reg >> (W-1)) ^ b;   reg = (reg << 1) mod 2^W;   if fb: reg ^= poly
 *    reg starts at init; the CRC is reg ^ xorout. The 72 bits of "123456789", MSB of each character
 *    first, give 0x29B1 for (16, 0x1021, 0xFFFF, 0) and 0x0376E6E7 for (32, 0x04C11DB7, 0xFFFFFFFF, 0).
 * 6. modem_crc_attach: bits is rows of nbits bytes, 1 <= nbits <= 65536; out rows of nbits + W
 *    bytes: out[f][i] = bits[f][i] & 1 for i < nbits, then the CRC of those nbits, most significant
 *    bit first. Nothing is written past nbits + W in a row.
 * 7. modem_crc_check: bits is rows of nbits + W bytes (the decoder's output); ok_in is NULL or
 *    nframes bytes; ok_out[f] = 1 iff (ok_in == NULL or ok_in[f] != 0) and the CRC of the first
 *    nbits equals the W bits that follow (bit 0 of each byte), else 0. ok_out == ok_in is allowed.
 *    Nothing is read back.
 *
 * Arguments, all five entries: bad P, pattern byte, weight, cols, Nm, E == 0, W, poly, init,
 * xorout, nbits, dtype, a row stride smaller than its row, a NULL pattern or (with nframes > 0) a
 * NULL buffer (ok and ok_in excepted), or input and output byte ranges that overlap (ok_out ==
 * ok_in excepted): INVALID_ARG, before any device is looked at. Then a bad ordinal is NO_DEVICE.
 * nframes == 0 succeeds and writes nothing. Every buffer is device memory of `device`, F16 and F32
 * buffers aligned to their element; anything else is INVALID_ARG. The calls are asynchronous on
 * `stream`. */
/* *kept = E for the pattern and Nm (host only, no device). */
modem_status modem_rm_kept(const uint8_t* pattern, uint32_t P, size_t nm, size_t* kept);
modem_status modem_rm_tx(const uint8_t* pattern, uint32_t P, uint32_t cols, const uint8_t* bits, size_t nframes, size_t nm,
                         size_t in_stride, uint8_t* out, size_t out_stride, int device, void* stream);
modem_status modem_rm_rx(const uint8_t* pattern, uint32_t P, uint32_t cols, int32_t dtype, const void* llr, size_t nframes,
                         size_t nm, size_t in_stride, const uint8_t* ok, void* out, size_t out_stride, int device, void* stream);
modem_status modem_crc_attach(uint32_t W, uint32_t poly, uint32_t init, uint32_t xorout, const uint8_t* bits, size_t nframes,
                              size_t nbits, size_t in_stride, uint8_t* out, size_t out_stride, int device, void* stream);
modem_status modem_crc_check(uint32_t W, uint32_t poly, uint32_t init, uint32_t xorout, const uint8_t* bits, size_t nframes,
                             size_t nbits, size_t in_stride, const uint8_t* ok_in, uint8_t* ok_out, int device, void* stream);

/* ---- synthetic input (GLUE): splitmix64 bit stream, one byte per bit ------------------- */
/* bit i = (word[i/64] >> (i%64)) & 1, word j = splitmix64 output j+1 from `seed`.
 * `out` must be a device pointer. */
modem_status modem_prng_bits(uint64_t seed, uint8_t* out, size_t nbits, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
