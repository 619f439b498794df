// rust-modem_amd/csrc/modem_scan_step.h — one step of the scanned phasors' f32 state recurrence
// (DMPSK / MFSK / BFSK: scan_bank in modem_tx.hip runs it, one lane per channel), with the
// constants and the division-free mod_trig it uses. Compiles for the device and for a plain host
// compiler (no HIP header needed there), so that tests/cpp/scan_step_host.cpp steps the same text
// against the oracle on the CPU. Host builds need -ffp-contract=off (the pragmas below are clang's).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MODEM_HD __host__ __device__ __forceinline__
#else
#define MODEM_HD inline
#endif

namespace mk {

#if !defined(__HIPCC__)
struct float2 { float x, y; };                 // HIP's float2, for the host build
#endif

constexpr float kTwoPi = 0x1.921fb6p+2f;   // std::f32::consts::PI * 2.0 (0x40c90fdb)
constexpr float kRcp2Pi = 0x1.45f306p-3f;  // fl(1 / kTwoPi)

// modem_phasor_kind of the sample-dependent phasors (include/modem_hip.h)
enum { PH_DCQPSK = 8, PH_DMPSK = 9, PH_CPFSK = 10, PH_MSK = 11, PH_MFSK = 12, PH_BFSK = 13 };

// mod_trig (util.rs:3-6: x - TWO_PI * floor(x / TWO_PI), the quotient an IEEE f32 division) for
// any f32 (the scan's phases can be negative), without the division: the carrier's division-free
// floor (phase_from_f: q0 = x RC, r = fma(-q0, TWO_PI, x), q1 = fma(r, RC, q0)) gives the same
// result bit for bit for every finite f32 once -0 is mapped to +0 (x + 0: the identity elsewhere;
// the reference gives +0 for -0, the division-free form -0). tools/mod_trig_check.cpp checks all
// 2^32 inputs offline: 0 mismatches; tests/cpp/scan_step_host.cpp (in the suite:
// tests/test_scan_states.py) compares this very function with the oracle's mod_trig over every
// exponent and around every multiple of 2 pi where the floor decides. The IEEE division was ~11
// dependent instructions of the scans' serial step (profiles/r06_scan_rate.txt).
MODEM_HD float mod_trig_ieee(float x) {
#pragma clang fp contract(off)
    const float xz = x + 0.0f;
    const float q0 = xz * kRcp2Pi;
    const float r = __builtin_fmaf(-q0, kTwoPi, xz);
    const float q1 = __builtin_fmaf(r, kRcp2Pi, q0);
    return xz - kTwoPi * __builtin_floorf(q1);
}

// DMPSK / MFSK / BFSK: update() runs at every symbol tick (modulator.rs:90-93) with the
// phase carried in f32 from symbol to symbol, so the states are a serial recurrence (no exact
// parallel form: the reachable f32 states do not close). One step, the reference's
// f32 operations in its order:
//   DMPSK (dmpsk.rs:29-33): phase = mod_trig(phase + sym * shift)
//   MFSK (mfsk.rs:68-75):   off = mod_trig(off + (cur - next) * dev * s); cur = next
//   BFSK (bfsk.rs:42-53):   on a change of bit, phase = mod_trig(phase + (b ? -dev*s : dev*(s-1)))
// s (su) is the carrier sample index after Carrier::next at the symbol's first sample.
struct ScanK {
    int kind;
    float shift, freq, max;
    int map;
    template <typename P>                      // P: TxParams (modem_internal.h)
    MODEM_HD static ScanK of(const P& p) { return ScanK{p.ph_kind, p.ph_shift, p.ph_freq, p.ph_max, p.ph_map}; }
};
template <int KIND>
MODEM_HD float2 scan_step(const ScanK& k, float2 st, uint32_t idx, uint64_t su) {
#pragma clang fp contract(off)
    if (KIND == PH_DMPSK) {
        st.x = mod_trig_ieee(st.x + (float)idx * k.shift);
    } else if (KIND == PH_MFSK) {
        const float next = k.map ? (float)(2 * (int)idx) : (float)(2 * (int)idx - (int)k.max);
        st.y = st.y + (st.x - next) * k.freq * (float)su;
        st.y = mod_trig_ieee(st.y);
        st.x = next;
    } else {                                   // BFSK: st = (phase, prev bit)
        const float b = (float)(idx & 1u);
        if (b != st.y) {
            const float d = b == 1.0f ? -(k.freq * (float)su) : k.freq * (float)(su - 1u);
            st.x = mod_trig_ieee(st.x + d);
            st.y = b;
        }
    }
    return st;
}

}  // namespace mk
