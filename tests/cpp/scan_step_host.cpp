// tests/cpp/scan_step_host.cpp — the scanned phasors' recurrence (rust-modem_amd/csrc/
// modem_scan_step.h: mod_trig_ieee, scan_step<KIND>, the very text the device kernels compile)
// on the CPU against the oracle, bit for bit. No GPU. Built and run by tests/test_scan_states.py:
//   g++ -O2 -std=c++17 -ffp-contract=off -Wno-unknown-pragmas -I rust-modem_amd/csrc -I oracle
//       tests/cpp/scan_step_host.cpp -L oracle/_build -lmodem_oracle
//   scan_step_host mod_trig        mod_trig_ieee(x) == or_mod_trig(x) over a structured input set
//   scan_step_host steps FILE      scan_step<KIND> next to or_phasor_update over the streams in FILE
// Exit status 1 at the first mismatch, with the input that produced it on stderr.
//
// FILE: per stream one line
//   NAME KIND BPS AMP PHASE SHIFT FREQ MAP S0 SPS NSYM BITS
// KIND 9 DMPSK / 12 MFSK / 13 BFSK; AMP .. FREQ the f32 parameters as hexadecimal bit patterns;
// BITS a string of NSYM * BPS characters 0 / 1.
#include <cinttypes>
#include <cmath>
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "modem_oracle.h"
#include "modem_scan_step.h"

static uint32_t bits_of(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static float float_of(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }

static uint64_t g_checked = 0;
static bool check_mod_trig(float x) {
    ++g_checked;
    const float a = or_mod_trig(x), b = mk::mod_trig_ieee(x);
    if (bits_of(a) == bits_of(b) || (std::isnan(a) && std::isnan(b))) return true;
    std::fprintf(stderr, "mod_trig mismatch: x = 0x%08x (%a): oracle 0x%08x (%a), mod_trig_ieee 0x%08x (%a)\n",
                 bits_of(x), x, bits_of(a), a, bits_of(b), b);
    return false;
}

// the nine f32 values within +-4 ulp of c
static bool check_around(float c) {
    float lo = c, hi = c;
    if (!check_mod_trig(c)) return false;
    for (int i = 0; i < 4; ++i) {
        lo = std::nextafterf(lo, -INFINITY);
        hi = std::nextafterf(hi, INFINITY);
        if (!check_mod_trig(lo) || !check_mod_trig(hi)) return false;
    }
    return true;
}

static bool check_multiple(double k) {
    // k * 2 pi in double, with pi itself and with the f32 constant the reference divides by
    return check_around((float)(k * 6.283185307179586476925)) && check_around((float)(k * (double)mk::kTwoPi));
}

static int run_mod_trig() {
    uint64_t s = 0x5CA45EED0001ull;                       // splitmix64
    auto next = [&s] {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    for (uint32_t e = 0; e < 256; ++e)                    // e = 255: inf and NaNs (both NaN: equal)
        for (uint32_t sign = 0; sign < 2; ++sign) {
            for (int i = 0; i < 2048; ++i)
                if (!check_mod_trig(float_of((sign << 31) | (e << 23) | (uint32_t)(next() & 0x7fffffu)))) return 1;
            if (!check_mod_trig(float_of((sign << 31) | (e << 23))) ||                 // the ends of the binade
                !check_mod_trig(float_of((sign << 31) | (e << 23) | 0x7fffffu)))
                return 1;
        }
    const float special[] = {0.0f, -0.0f, float_of(1u), float_of(0x007fffffu), FLT_MIN, FLT_MAX};
    for (float x : special)
        if (!check_mod_trig(x) || !check_mod_trig(-x)) return 1;
    for (int k = 1; k <= 4096; ++k)
        if (!check_multiple((double)k) || !check_multiple(-(double)k)) return 1;
    for (int j = 13; j <= 40; ++j)
        for (int d = -3; d <= 3; ++d) {
            const double k = std::ldexp(1.0, j) + (double)d;
            if (!check_multiple(k) || !check_multiple(-k)) return 1;
        }
    std::printf("mod_trig_ieee == or_mod_trig on %" PRIu64 " inputs\n", g_checked);
    return 0;
}

template <int KIND>
static bool run_stream(const std::string& name, uint32_t bps, float amp, float phase, float shift, float freq,
                       int map, uint64_t s0, uint64_t sps, const std::vector<uint8_t>& bits, size_t nsym) {
    or_phasor p;
    int rc;
    if (KIND == mk::PH_DMPSK) rc = or_dmpsk_new(&p, bps, amp, phase, shift);
    else if (KIND == mk::PH_MFSK) rc = or_mfsk_new(&p, bps, freq, amp, map);
    else rc = or_bfsk_new(&p, freq, amp);
    if (rc != 0) { std::fprintf(stderr, "%s: the oracle refuses the parameters\n", name.c_str()); return false; }
    const mk::ScanK k{KIND, shift, freq, (float)((1u << bps) - 1u), map};
    // the handle's initial state (modem_tx_create): DMPSK its phase, MFSK / BFSK zeros
    mk::float2 st{KIND == mk::PH_DMPSK ? phase : 0.0f, 0.0f};
    for (size_t m = 0; m < nsym; ++m) {
        uint32_t idx = 0;                                  // bytes_to_bits, MSB first (digital/util.rs:5-11)
        for (uint32_t b = 0; b < bps; ++b) idx |= (uint32_t)(bits[m * bps + b] & 1u) << (bps - 1 - b);
        const uint64_t su = s0 + m * sps + 1u;
        const mk::float2 before = st;
        st = mk::scan_step<KIND>(k, st, idx, su);
        or_phasor_update(&p, su, &bits[m * bps], bps);
        float wx, wy;
        bool ok;
        if (KIND == mk::PH_DMPSK) { wx = p.phase; wy = st.y; ok = bits_of(st.x) == bits_of(wx); }
        else if (KIND == mk::PH_MFSK) { wx = p.cur_coef; wy = p.phase; ok = bits_of(st.x) == bits_of(wx) && bits_of(st.y) == bits_of(wy); }
        else { wx = p.phase; wy = (float)p.prev; ok = bits_of(st.x) == bits_of(wx) && bits_of(st.y) == bits_of(wy); }
        if (!ok) {
            std::fprintf(stderr,
                         "%s: symbol %zu (index %u, s = %" PRIu64 "): state before (0x%08x, 0x%08x) -> scan_step "
                         "(0x%08x, 0x%08x) = (%a, %a), oracle (0x%08x, 0x%08x) = (%a, %a)\n",
                         name.c_str(), m, idx, su, bits_of(before.x), bits_of(before.y), bits_of(st.x), bits_of(st.y),
                         st.x, st.y, bits_of(wx), bits_of(wy), wx, wy);
            return false;
        }
    }
    return true;
}

static int run_steps(const char* path) {
    std::ifstream f(path);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
    std::string line;
    size_t streams = 0, symbols = 0;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        std::string name, sbits;
        int kind = 0, map = 0;
        uint32_t bps = 0, a = 0, ph = 0, sh = 0, fr = 0;
        uint64_t s0 = 0, sps = 0;
        size_t nsym = 0;
        is >> name >> kind >> bps >> std::hex >> a >> ph >> sh >> fr >> std::dec >> map >> s0 >> sps >> nsym >> sbits;
        if (!is || bps < 1 || bps > 8 || sbits.size() != nsym * bps) {
            std::fprintf(stderr, "bad stream line: %.60s\n", line.c_str());
            return 2;
        }
        std::vector<uint8_t> bits(sbits.size());
        for (size_t i = 0; i < sbits.size(); ++i) bits[i] = (uint8_t)(sbits[i] == '1');
        bool ok;
        switch (kind) {
        case mk::PH_DMPSK: ok = run_stream<mk::PH_DMPSK>(name, bps, float_of(a), float_of(ph), float_of(sh), float_of(fr), map, s0, sps, bits, nsym); break;
        case mk::PH_MFSK: ok = run_stream<mk::PH_MFSK>(name, bps, float_of(a), float_of(ph), float_of(sh), float_of(fr), map, s0, sps, bits, nsym); break;
        case mk::PH_BFSK: ok = run_stream<mk::PH_BFSK>(name, bps, float_of(a), float_of(ph), float_of(sh), float_of(fr), map, s0, sps, bits, nsym); break;
        default: std::fprintf(stderr, "%s: kind %d is not a scanned phasor\n", name.c_str(), kind); return 2;
        }
        if (!ok) return 1;
        ++streams;
        symbols += nsym;
    }
    std::printf("scan_step == or_phasor_update on %zu streams, %zu symbols\n", streams, symbols);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "mod_trig") == 0) return run_mod_trig();
    if (argc == 3 && std::strcmp(argv[1], "steps") == 0) return run_steps(argv[2]);
    std::fprintf(stderr, "usage: %s mod_trig | steps FILE\n", argv[0]);
    return 2;
}
