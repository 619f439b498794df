// rust-modem_amd/csrc/modem_internal.h — kernel parameter blocks and launchers shared by
// modem_kernels.hip (device code) and capi_*.cpp (the C ABI). Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>

namespace mk {

// The RX MFMA kernels walk a call's tiles in rounds from the top down (rx_mfma_body), so the
// last samples a TX launch wrote are the first the RX reads. The TX store policy relies on it
// (capi_tx.cpp tx_nt_below: a single-channel launch of <= 256 MiB keeps its second half
// cacheable); rx_mfma_body asserts it. Changing the RX walk means revisiting that policy.
constexpr bool kRxTilesTopDown = true;

// One TX launch: symbols [0, nsym) of this call -> samples [0, nsym*sps).
struct TxParams {
    const uint8_t* bits;     // this call's bits, one byte per bit (device)
    const uint8_t* carry;    // ncarry leftover bits of the previous call (device)
    uint8_t* carry_new;      // leftover bits after this call (other buffer)
    const float2* hist;      // K-1 complex symbol values preceding symbol 0 (device)
    float2* hist_new;        // K-1 values preceding the next call's symbol 0
    const float2* lut;       // 2^bps complex points (device)
    const float* taps;       // polyphase taps, taps[t*sps + p] = h[p + sps*t], K*sps floats
    const float* taps_q;     // Q-rail taps (the I taps delayed by the Q offset), or null: = taps
    void* out;               // f32 or f16 samples (layout per out_mode)
    int64_t nt_below;        // tx_mfma: full sub-tiles of call samples < nt_below store non-temporally
    uint64_t s0;             // carrier sample of output sample 0
    int64_t nsym;            // symbols this call emits
    int64_t nsym_valid;      // symbols < nsym_valid are data, the rest are zero (flush)
    int64_t nbits;           // bits in `bits`
    int32_t ncarry;          // bits in `carry`
    int32_t ncarry_new;      // bits to leave in `carry_new`
    int32_t update_carry;    // 0 during flush
    int32_t bps;
    int32_t sps;             // runtime samples/symbol (generic kernel)
    int32_t K;               // taps per polyphase branch = ceil(ntaps / sps)
    int32_t fast_bits;       // ncarry == 0, bps in {1,2,4,8}, bits aligned to bps bytes
    int32_t exact_idx;       // every carrier index of this call is < 2^53 (exact as f64)
    int32_t idx46;           // ... and < 2^46 (tx_mfma's exact f32 index split, emit_full)
    float w;                 // Freq::sample_freq()
    // tx_mfma (split-f16 FIR): LUT as (re_hi, re_lo, im_hi, im_lo) halves of lut * 2^lut_scale_exp,
    // B fragments hold taps * 2^tap_scale_exp; lead = symbols before this call, mod 16/sps.
    const void* lut_h;
    int32_t lut_scale_exp;
    int32_t tap_scale_exp;
    int32_t lead;
    // levels: every LUT component is an integer multiple of one scale s, folded into the taps;
    // lut_h then holds the exact f16 integer levels (lo halves zero) and a symbol value v of the
    // history maps to the level rint(v * level_inv), level_inv = 1/s.
    int32_t levels;
    float level_inv;
    // tx_phasor (sample-dependent phasors, sample-and-hold): kind (modem_phasor_kind), the
    // symbols emitted before this call (DCQPSK parity), amplitude, CPFSK frequency, MSK
    // samples per bit, Q offset (0 or sps/2). `lut` then holds the DCQPSK table
    // (even-count block, then odd-count block); `hist[0].x` the index of the symbol before
    // symbol 0 (the offset Q rail's bits).
    int32_t ph_kind;
    uint64_t sym0;
    float ph_amp;
    float ph_freq;
    int32_t ph_spb;
    int32_t q_off;
    // DMPSK / MFSK / BFSK: per-symbol states of this call (tx_scan writes, tx_phasor reads),
    // the DMPSK shift, the MFSK map and max symbol. The handle state (DMPSK phase; MFSK
    // cur_coef, phase_offset; BFSK phase, prev bit) is hist[0] -> hist_new[0].
    float2* scan;
    float ph_shift;
    int32_t ph_map;
    float ph_max;
};

// One RX launch: input samples [0, N) (stream indices n_start ..), outputs k_first ..
struct RxParams {
    const void* x;           // this chunk: N complex samples (f32x2 or f16x2)
    const void* hist;        // HL samples preceding x (same dtype); zeros before the stream
    void* hist_new;          // HL samples preceding the next chunk
    void* out_iq;            // decimated filter outputs (f32x2 or f16x2), may be null
    uint8_t* out_sym;        // decisions, may be null
    const float* taps;       // polyphase taps, taps[b*K + t] = h[b + decim*t], decim*K floats
    const float2* slut;      // NEAREST slicer LUT (device)
    int64_t N;
    int64_t n_start;         // stream index of x[0]
    uint64_t c0;             // carrier sample of stream index 0
    int64_t k_first;         // first kept instant: n = k*decim + D
    int64_t nout;            // kept instants in this call
    int32_t K;               // taps per polyphase branch
    int32_t L;               // ntaps (generic kernel)
    int32_t HL;              // history length = K*decim - 1
    int32_t D;               // decim_offset
    int32_t decim;           // runtime decimation (generic kernel)
    int32_t x_aligned16;     // x is 16-byte aligned (pair loads)
    int32_t exact_idx;
    int32_t slicer_kind;
    int32_t bps;
    int32_t bits_per_carrier;
    float inv_scale;
    float max_symbol;
    float w;
    int32_t tap_scale_exp;   // rx_mfma: tables hold h * 2^tap_scale_exp
    float phase_offset;      // PLL offset added to the carrier phase (demodulator.rs:50)
    int32_t idx46;           // every carrier index of this call is < 2^46 (rx_mfma's f32 index split)
    const int* ka_in;        // rx_mfma: staging exponent the previous call ended with (INT_MIN: none)
    int* ka_out;             // rx_mfma: the one this call ends with (written with its last tile)
};

struct FirParams {
    const float* x;
    const float* hist;       // L-1 samples preceding x
    float* hist_new;
    float* y;
    const float* taps;       // h[k], L floats
    int64_t N;
    int32_t L;
};

// Launchers return hipSuccess or the launch error. They pick a specialised kernel for the
// common samples-per-symbol values and a generic one otherwise.
hipError_t launch_tx(const TxParams& p, int sps, int dtype, int out_mode, hipStream_t s);
// Sample-dependent phasors (DCQPSK, CPFSK, MSK; DMPSK, MFSK, BFSK after a serial symbol-state
// scan), sample-and-hold: tx_scan + tx_phasor.
// scanned: the states are already in p.scan (a batch's tx_scan_batch ran), only tx_phasor runs.
hipError_t launch_tx_phasor(const TxParams& p, int dtype, int out_mode, hipStream_t s, bool scanned = false);
// The serial state scan of DMPSK / MFSK / BFSK for nch channels of one phasor kind at once, one
// lane per channel (dps: their TxParams in device memory, p.scan set).
hipError_t launch_tx_scan_batch(const TxParams* dps, int nch, int kind, hipStream_t s);
// TX FIR on the matrix cores (tx_mfma, split-f16 MFMA): 32-symbol k-steps for (sps, K), or 0
// when no variant fits; bfrag = per-lane B fragments [ksteps][hi, lo][64 lanes][8 halves].
int tx_mfma_ksteps(int sps, int K);
// Channel batches (modem_tx_process_batch / modem_rx_process_batch): up to kBatchMax
// independent handles of one configuration in one launch; the launcher sets g, the
// workgroups per channel (workgroup b serves channel b / g), rot and xc (xcd_chunk of g).
constexpr int kBatchMax = 8;
struct TxBatch { TxParams p[kBatchMax]; int32_t nch; int32_t g; int32_t rot; int32_t xc; };
struct RxBatch { RxParams p[kBatchMax]; int32_t nch; int32_t g; int32_t rot; int32_t xc; };
// The per-channel rotation of a batch launch's workgroups (a multiple of 8, so that every tile
// keeps its XCD slot: blocks b and b + 8 share an XCD); 0 when g is not a multiple of 8.
// MODEM_BATCH_ROT=0 in the environment turns it off (A/B).
inline int32_t batch_rot(int32_t g, int32_t nch) {
    static const bool on = [] { const char* e = std::getenv("MODEM_BATCH_ROT"); return !e || e[0] != '0'; }();
    return on && g % 8 == 0 && 8 * (nch - 1) < g ? 8 : 0;
}
// mixed-carrier I/Q output only (OUT_IQ_MIXED); dtype 0 f32, 1 f16
hipError_t launch_tx_mfma_batch(const TxBatch& b, int sps, int nks, const void* bfrag, int dtype, hipStream_t s);
// complex mix only (MIX_COMPLEX); in and out of one dtype
hipError_t launch_rx_mfma_batch(const RxBatch& b, int decim, int nks, const void* tables, int dtype, hipStream_t s);
hipError_t launch_tx_mfma(const TxParams& p, int sps, int nks, const void* bfrag, int dtype,
                          int out_mode, hipStream_t s);
// RX matched filter on the matrix cores (rx_mfma, split-f16 MFMA): 32-sample k-steps for
// (decim, ntaps), or 0 when no variant fits.
int rx_mfma_ksteps(int decim, int L);
// Its tap tables: rx_mfma_table_copies(decim) copies q of the reversed taps
// T[x] = h[W - 1 - x] * 2^tap_scale_exp (W = 32*nks), copy q holding T[y + q*gcd(decim, 8)],
// each as hi then lo f16 halves of rx_mfma_table_len(decim, nks) entries.
constexpr int rx_mfma_table_copies(int decim) {
    return 8 / (decim % 8 == 0 ? 8 : decim % 4 == 0 ? 4 : decim % 2 == 0 ? 2 : 1);
}
// Padded so that the 16 lanes of every ds_read_b128 lane group read distinct LDS bank quads
// across the NC copies (bank model of MI355X_MICROARCH.md §LDS, checked by tests/test_lds_banks.py):
// len % 64 == 32 halves when decim % 8 == 4, else 16.
constexpr int rx_mfma_table_len(int decim, int nks) {
    const int n = (32 * nks + 15 * decim + 8 + 7) & ~7;
    const int r = decim % 8 == 4 ? 32 : 16;
    return n + ((r - (n % 64)) % 64 + 64) % 64;
}
hipError_t launch_rx_mfma(const RxParams& p, int decim, int nks, const void* tables, int in_dtype,
                          int out_dtype, int mix, hipStream_t s);
hipError_t launch_rx(const RxParams& p, int decim, int in_dtype, int out_dtype, int mix,
                     hipStream_t s);
// One loopback period (TX into the sample buffer rp.x == tp.out, then RX over it, complex
// mix, in and out of one dtype) as one persistent launch (modem_chain.hip); hipErrorNotSupported
// when the filters or the call's geometry have no fused form (run the two launches then);
// *form = 1 (chain_mfma) or 2 (chain_small: one RX tile per workgroup, LDS hand-off).
hipError_t launch_chain_mfma(const TxParams& tp, int sps, int nks_t, const void* bfrag, const RxParams& rp,
                             int nks_r, const void* tables, int dtype, hipStream_t s, int* form);
// The matrix-core variants by element types, instantiated in their own translation units
// (modem_txm_*.hip: OM = OUT_IQ_MIXED / BASEBAND / REAL, OutT = float / __half; modem_rxm_*.hip:
// MIX = MIX_COMPLEX / MIX_REFERENCE_REAL, InT, OutT = float / __half) and dispatched from
// launch_tx_mfma* / launch_rx_mfma* (hipErrorInvalidValue: no variant for the shape).
template <int OM, typename OutT>
hipError_t txm_sel(const TxParams& p, int sps, int nks, const void* bfrag, hipStream_t s);
template <typename OutT>
hipError_t txm_sel_batch(const TxBatch& b, int sps, int nks, const void* bfrag, hipStream_t s);
template <typename InT, int MIX, typename OutT>
hipError_t rxm_sel(const RxParams& p, int decim, int nks, const void* tables, hipStream_t s);
template <typename T>
hipError_t rxm_sel_batch(const RxBatch& b, int decim, int nks, const void* tables, hipStream_t s);
hipError_t launch_fir(const FirParams& p, hipStream_t s);
// Soft demapper (modem_demap.hip): per-bit max-log LLRs of nsym received points, one lane per
// symbol. General path: tab = the 2^bps (i, q) points. Axis path (a product grid with an even
// bit split, checked by modem_demap_create): tab = the 2^(bps/2) I levels, then the Q levels.
struct DemapParams {
    const void* iq;          // nsym interleaved (i, q), f32 or f16
    void* llr;               // nsym * bps values, symbol k's bps values contiguous, MSB first
    const float* tab;        // device table (see above)
    int64_t nsym;
    float scale;
    int32_t bps;
};
// out_dtype: 0 f32, 1 f16 (saturating), 3 i8 (rint of the value clamped to +-127)
hipError_t launch_demap(const DemapParams& p, bool axis, int in_dtype, int out_dtype, hipStream_t s);
// Noncoherent detectors (modem_noncoh.hip). out_dtype as launch_demap's; either output may be null.
// Differential detector: z[k] = r[k] * conj(r[k-1]), c(s) = z.re * tab[2s] + z.im * tab[2s+1];
// r[-1] = *prev, and the lane of symbol nsym-1 leaves r[nsym-1] (widened to f32) in *prev_new.
struct DiffParams {
    const void* iq;          // nsym interleaved (i, q), f32 or f16
    const float2* prev;      // the point before iq[0] (device)
    float2* prev_new;        // the point before the next call's iq[0] (the handle's other slot)
    const float* tab;        // 2^bps (cos, sin) pairs (device)
    uint8_t* sym;            // nsym decisions
    void* llr;               // nsym * bps values, MSB first
    int64_t nsym;
    float scale;
    int32_t bps;
};
hipError_t launch_diff(const DiffParams& p, int in_dtype, int out_dtype, hipStream_t s);
// Tone-bank energy detector: symbol k of this call covers the samples [k*sps, (k+1)*sps) of the
// logical stream `carry` (ncarry < sps samples) followed by `in` (n samples); the samples after
// the last whole symbol go to carry_new. tw: the twiddles e^{-j omega[m] i} as (cos, -sin), tone m
// at sample i in entry fsk_tw_index(bps, sps, m, i): tones in groups of kFskTM, a group's tones
// of one sample contiguous (a wave works on one group: wave-uniform, scalar loads).
constexpr int kFskTM = 16;
constexpr size_t fsk_tw_index(int bps, int sps, int m, int i) {
    const int M = 1 << bps, TM = M < kFskTM ? M : kFskTM;
    return ((size_t)(m / TM) * sps + i) * TM + m % TM;
}
struct FskParams {
    const void* in;          // n complex samples, f32 or f16
    const void* carry;       // ncarry samples of the same dtype
    void* carry_new;
    const float2* tw;
    uint8_t* sym;            // nsym decisions
    void* llr;               // nsym * bps values, MSB first
    float* energy;           // nsym * 2^bps tone energies
    int64_t n;
    int64_t nsym;            // whole symbols in carry + in
    int32_t ncarry;
    int32_t sps;
    int32_t bps;
    float scale;
};
hipError_t launch_fsk(const FskParams& p, int in_dtype, int out_dtype, hipStream_t s);
// Channel model (modem_chan.hip): y = gain * x * e^{j theta} + sig * w for the n samples of one call,
// passed by value. cnt0 = k + (n_abs + 1) * GOLDEN and ph0 = phase0 + step * n_abs for the call's
// first sample n_abs (64-bit wrap-around); align is set by the launcher (2: both buffers 16-byte
// aligned, 1: sample-aligned, 0: element-aligned).
struct ChanParams {
    const void* in;          // n interleaved (i, q), f32 or f16
    void* out;               // n interleaved (i, q), f32 or f16; may equal `in` when the dtypes do
    int64_t n;
    uint64_t cnt0;
    uint64_t ph0;
    uint64_t step;
    float gain;
    float sig;               // sqrt(n0)
    int32_t align;
};
// noise: sig != 0; rot: step != 0 or phase0 != 0. dtypes: 0 f32, 1 f16.
hipError_t launch_chan(const ChanParams& p, bool noise, bool rot, int in_dtype, int out_dtype, hipStream_t s);
// counts[0] += #{i: a[i] != b[i]}, counts[1] += sum popcount(a[i] ^ b[i]) (device pointers)
hipError_t launch_count_errors(const uint8_t* a, const uint8_t* b, size_t n, uint64_t* counts, hipStream_t s);
// Carrier synchronizer (modem_sync.hip), one modem_sync_process call, passed by value. The logical
// stream of the call is `carry || in`: ncarry symbols the handle kept, then the n new ones; its
// first nblk * B symbols are estimated (phi, q), unwrapped (th) and derotated (out), the rest
// (< B) goes to carry_new. state / state_new: {theta, Phi, d} of the last block before / after the
// call (d = theta_b - theta_{b-1} as the apply step uses it: 0 for the stream's first block).
// th has nblk + 1 entries: th[0] = theta before the call, th[1 + b] = theta of the call's block b.
struct SyncParams {
    const void* in;          // n interleaved (i, q) of the input dtype
    const void* carry;       // ncarry symbols of the input dtype, 16-byte aligned
    void* carry_new;         // the other carry slot
    void* out;               // nblk * B interleaved (i, q) of the output dtype
    uint64_t* phi;           // [nblk]     workspace: Phi of every block
    uint64_t* th;            // [nblk + 1] workspace
    float* q;                // [nblk]     workspace: quality of every block
    const uint64_t* state;
    uint64_t* state_new;
    int64_t n, nblk;
    uint64_t ref;            // ref_phase in 2^-64 turns
    float nrm;
    int32_t ncarry, lb, lm;
    int32_t first;           // no block was completed before this call: d of block 0 is 0
    int32_t flat;            // MODEM_SYNC_FLAT: s = 0
    int32_t in_align, out_align;   // set by the launcher: 2 = groups of 4 symbols 16-byte aligned, 1 = symbol-aligned, 0 = element-aligned
};
constexpr int kSyncState = 3;    // u64 words per state slot
// est + scan + apply (nblk > 0), or only the move of the leftover into carry_new (nblk == 0)
hipError_t launch_sync(const SyncParams& p, int in_dtype, int out_dtype, hipStream_t s);
// flush: the ncarry carried symbols, rotated on the last block's line extended (i -> i + B)
hipError_t launch_sync_flush(const SyncParams& p, int in_dtype, int out_dtype, hipStream_t s);
// Symbol timing synchronizer (modem_timing.hip), one modem_timing_process call, passed by value. The
// logical stream of the call is `pre || in`: the npre = H + carried samples the handle kept (H =
// 2 span N + 1 samples of history before the current block, always present, zeros at the start of
// a stream; then the samples of the incomplete block), then the n new ones. Block b of the call is
// the B N samples from index H + b B N; its taps reach back to index b B N. The first nblk blocks
// are estimated (phi, q), unwrapped (th) and interpolated (out); the last H + left samples of the
// logical stream go to pre_new. state / state_new: {D, Phi, d} of the last block before / after
// the call, as int64 (d = D_b - D_{b-1} as the apply step uses it: 0 for the stream's first block).
// th has nblk + 1 entries: th[0] = D before the call, th[1 + b] = D of the call's block b.
struct TimingParams {
    const void* in;          // n interleaved (i, q) samples of the input dtype
    const void* pre;         // npre samples of the input dtype, 16-byte aligned
    void* pre_new;           // the other slot
    void* out;               // nblk * B interleaved (i, q) of the output dtype
    uint32_t* phi;           // [nblk]     workspace: Phi of every block
    int64_t* th;             // [nblk + 1] workspace
    float* q;                // [nblk]     workspace: quality of every block
    const int64_t* state;
    int64_t* state_new;
    int64_t n, nblk;
    int32_t npre;            // H + carried
    int32_t lb, ln, span;    // log2 B, log2 N, span in symbols
    int32_t first;           // no block was completed before this call: d of block 0 is 0
    int32_t flat;            // MODEM_TIMING_FLAT: s = 0
    int32_t nflush;          // flush: symbols to emit
    int32_t in_align, out_align;   // set by the launcher: 2 = wide accesses aligned, 1 = sample-aligned, 0 = element-aligned
};
constexpr int kTimingState = 3;  // int64 words per state slot
// est + scan + apply (nblk > 0), or only the move of the logical stream's tail into pre_new (nblk == 0)
hipError_t launch_timing(const TimingParams& p, int in_dtype, int out_dtype, hipStream_t s);
// flush: nflush symbols on the last block's line extended (i -> i + B); pre_new gets H zero samples
hipError_t launch_timing_flush(const TimingParams& p, int in_dtype, int out_dtype, hipStream_t s);
// Frame synchronizer (modem_frame.hip), one modem_frame_process or modem_frame_flush call, passed by
// value. The logical stream of the call is `carry || in`: ncarry symbols the handle kept (the last
// min(T, 2W + L - 1) of its window), then the n new ones, nlog = ncarry + n in all; logical
// position 0 is stream symbol `base`. Positions 0 .. nlog - L exist; d0 .. d1 - 1 are decided by
// this call (tile t covers d0 + 256 t ..). cnt / off: hits per tile and their exclusive prefix sum;
// rec: maxh records {c.re, c.im, e, offset in the tile} per tile, maxh = ceil(256 / (W + 1)) (hits
// are more than W apart). The emit step writes the first min(*count, cap) hits and moves the last
// `keep` logical symbols into carry_new.
struct FrameParams {
    const void* in;          // n interleaved (i, q) of the input dtype
    const void* carry;       // ncarry symbols of the input dtype, 16-byte aligned
    void* carry_new;         // the other carry slot
    const float* uw;         // L (re, im) pairs
    uint32_t* cnt;           // [ntiles] workspace
    uint64_t* off;           // [ntiles] workspace
    float* rec;              // [ntiles * maxh * 4] workspace
    uint64_t* pos;           // [cap]
    uint32_t* phi;           // [cap] or NULL
    float* metric;           // [cap] or NULL
    uint64_t* count;
    int64_t n, d0, d1, ntiles;
    uint64_t base, cap;
    float t2, eu;
    int32_t ncarry, L, W, maxh, keep;
    int32_t in_align;        // set by the launcher: 1 = symbol-aligned, 0 = element-aligned
};
constexpr int kFrameTile = 256;  // decided positions per workgroup
constexpr int kFrameMaxL = 256, kFrameMaxW = 256;
// correlate + pick (ntiles > 0), scan (always: it writes *count), emit + carry
hipError_t launch_frame(const FrameParams& p, int in_dtype, hipStream_t s);
// Frame gather (modem_frame.hip): row f < cap of `out` = len symbols from in[pos[f] - base + skip],
// rotated by the multiple of 1 / M turn nearest phi[f] (M = 2^lm; phi NULL or lm 0: none), or zeros
// and ok[f] = 0 when f >= min(*count, cap) or the symbols are not all inside [base, base + n).
struct FrameGatherParams {
    const void* in;
    void* out;
    uint8_t* ok;
    const uint64_t* pos;
    const uint32_t* phi;
    const uint64_t* count;
    uint64_t n, base, cap;
    uint32_t skip, len;
    int32_t lm;
    int32_t in_elem, out_elem;   // set by the launcher: the buffer is only element-aligned
};
hipError_t launch_frame_gather(const FrameGatherParams& p, int in_dtype, int out_dtype, hipStream_t s);
// Convolutional code (modem_fec.hip), include/modem_hip.h "Convolutional code". The encoder: row f
// of `bits` (nbits bytes, bit 0 of each) into row f of `out` (n * T bytes), T = nbits + K - 1 with
// the tail, else nbits; g by value.
struct ConvEncodeParams {
    const uint8_t* bits;
    uint8_t* out;
    uint64_t nframes, nbits, T, in_stride, out_stride;
    uint32_t g[3];
    int32_t K, n;
};
hipError_t launch_conv_encode(const ConvEncodeParams& p, hipStream_t s);
// The Viterbi decoder, one modem_viterbi_process call, passed by value. table: the S branch words
// of the code (modem_fec_math.h, fec_branch_word), the handle's only device memory. llr: nframes rows
// of n * T values, row stride `stride` elements; out: rows of nbits bytes; ok, metric: NULL or
// nframes entries. A wave decodes 64 / S frames (S <= 64) or one frame with S / 64 states per lane.
struct ViterbiParams {
    const void* llr;
    const uint8_t* ok;
    const uint32_t* table;
    uint8_t* out;
    int32_t* metric;
    uint64_t nframes, stride, out_stride;
    float qscale;
    int32_t K, n, tail;
    int32_t nbits, T;
};
// in_dtype: 0 F32, 1 F16, 3 I8
hipError_t launch_viterbi(const ViterbiParams& p, int in_dtype, hipStream_t s);
// Rate matching (modem_ratematch.hip), include/modem_hip.h "Rate matching and frame check". mask:
// bit i is pattern[i]; w its weight; E the kept indices below nm; rows, cl of the interleaver of C
// columns. tx: in rows of nm bytes, out rows of E bytes; rx: in rows of E elements, out rows of nm
// (strides in elements). Both set by the caller (capi_ratematch.cpp) from modem_ratematch_math.h.
struct RmParams {
    const void* in;
    void* out;
    uint64_t nframes, in_stride, out_stride, mask;
    uint32_t P, w, nm, E, C, rows, cl;
};
hipError_t launch_rm_tx(const RmParams& p, hipStream_t s);
// elem: bytes of a value, 1, 2 or 4
hipError_t launch_rm_rx(const RmParams& p, int elem, hipStream_t s);
// The CRC: rows of nbits message bytes (bit 0 of each). attach: out rows of nbits + W bytes;
// check: in rows of nbits + W bytes, ok_in NULL or nframes bytes, ok_out nframes bytes.
struct CrcParams {
    const uint8_t* in;
    uint8_t* out;                // attach: the rows; check: ok_out
    const uint8_t* ok_in;
    uint64_t nframes, in_stride, out_stride;
    uint32_t nbits, W, poly, init, xorout;
};
hipError_t launch_crc_attach(const CrcParams& p, hipStream_t s);
hipError_t launch_crc_check(const CrcParams& p, hipStream_t s);
hipError_t launch_phases(float w, uint64_t s0, size_t n, float* out, hipStream_t s);
hipError_t launch_prng_bits(uint64_t seed, uint8_t* out, size_t nbits, hipStream_t s);

// Largest tap count the kernels accept (LDS budget).
constexpr int kMaxTaps = 4096;
// Zero steps appended to the polyphase tap buffers (look-ahead loads of the next chunk).
constexpr int kTapPad = 16;

}  // namespace mk
