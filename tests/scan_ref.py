"""Shared by tests/test_scan_states.py (CPU) and tests/test_gpu_scan_states.py (GPU): the scanned
phasors' parameter sets, their input streams, the oracle's per-symbol state sequence and an
independent numpy float32 restatement of the three update rules.

A phasor is a plain tuple, so that a bank can mix parameters within one kind:
    ("dmpsk", bps, amplitude, phase, shift)      dmpsk.rs:16-23
    ("mfsk", bps, (hz, sr), amplitude, map)      mfsk.rs:46-59, map 1 = IncreaseMap, 0 = DefaultMap
    ("bfsk", (hz, sr), amplitude)                bfsk.rs:12-20
A state is one (x, y) pair per symbol, as modem_tx_scan_states documents it: DMPSK (phase, -),
MFSK (cur_coef, phase_offset), BFSK (phase, previous bit).
"""
import functools

import numpy as np

import __graft_entry__ as graft

F = np.float32
TWO_PI = np.uint32(0x40C90FDB).view(np.float32)     # std::f32::consts::PI * 2.0
RC = np.uint32(0x3E22F983).view(np.float32)         # fl(1 / TWO_PI)

SPS = 4
NSYM = 4096
S0S = (3, (1 << 24) + 5, (1 << 32) + 12345)
SEED = 0x5CA45000

KINDS = {
    "dqpsk": ("dmpsk", 2, 1.0, 0.7853982, 1.5707964),
    "dbpsk": ("dmpsk", 1, 1.0, 0.7853982, 3.1415927),
    "d8psk": ("dmpsk", 3, 1.0, 0.1, 0.7853982),
    "mfsk": ("mfsk", 4, (50, 10000), 1.0, 1),
    "mfsk_default": ("mfsk", 3, (120, 10000), 0.5, 0),
    "bfsk": ("bfsk", (200, 10000), 1.0),
}
COLUMNS = {"dmpsk": [0], "mfsk": [0, 1], "bfsk": [0, 1]}     # the state columns that are specified


def bps_of(spec):
    return 1 if spec[0] == "bfsk" else spec[1]


def product_phasor(m, spec):
    if spec[0] == "dmpsk":
        return m.DMPSK(*spec[1:])
    if spec[0] == "mfsk":
        return m.MFSK(spec[1], m.Freq(*spec[2]), spec[3], "increase" if spec[4] else "default")
    return m.BFSK(m.Freq(*spec[1]), spec[2])


def oracle_phasor(o, spec):
    if spec[0] == "dmpsk":
        return o.new_phasor(o.DMPSK, *spec[1:])
    if spec[0] == "mfsk":
        return o.new_phasor(o.MFSK, spec[1], o.sample_freq(*spec[2]), spec[3], spec[4])
    return o.new_phasor(o.BFSK, o.sample_freq(*spec[1]), spec[2])


def oracle_states(o, spec, bits, s0, sps=SPS):
    """The oracle's state after every symbol tick: or_phasor_update with the carrier sample after
    Carrier::next at the symbol's first sample (modulator.rs:85-93), s = s0 + m * sps + 1."""
    p = oracle_phasor(o, spec)
    bps = bps_of(spec)
    n = len(bits) // bps
    out = np.zeros((n, 2), F)
    for m in range(n):
        o.phasor_update(p, s0 + m * sps + 1, bits[m * bps:(m + 1) * bps])
        out[m] = (p.cur_coef, p.phase) if spec[0] == "mfsk" else (p.phase, p.prev if spec[0] == "bfsk" else 0.0)
    return out


# One seed per kind, chosen so that the test_streams_expose_* tests of test_scan_states.py hold (a
# wrong step differs from the oracle on the stream): a condition that the reference alone decides.
SEEDS = {"bfsk": SEED + 2, "d8psk": SEED + 16, "dbpsk": SEED + 17, "dqpsk": SEED + 18, "mfsk": SEED + 19,
         "mfsk_default": SEED + 20}


def stream_bits(o, name):
    """NSYM symbols and one leftover bit (none where a symbol is one bit); one stream per kind,
    the same at every s0."""
    bps = bps_of(KINDS[name])
    return o.prng_bits(SEEDS[name], bps * NSYM + (1 if bps > 1 else 0))


@functools.lru_cache(maxsize=None)
def case(name, s0):
    """(bits, oracle states) of one (kind, s0), computed once and shared (read-only)."""
    o = graft.oracle()
    bits = stream_bits(o, name)
    st = oracle_states(o, KINDS[name], bits, s0)
    for a in (bits, st):
        a.setflags(write=False)
    return bits, st


def same_bits(got, want, cols):
    """Bitwise equality of the specified state columns."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32)[:, cols], want.view(np.uint32)[:, cols])


def first_difference(got, want, cols):
    """'symbol m: got (bits) want (bits)' of the first differing symbol, for assertion messages."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = np.nonzero((got.view(np.uint32)[:, cols] != want.view(np.uint32)[:, cols]).any(axis=1))[0]
    if len(bad) == 0:
        return "equal"
    k = int(bad[0])
    hx = lambda a: "(" + ", ".join(f"0x{int(v):08x}" for v in a.view(np.uint32)) + ")"   # noqa: E731
    prev = hx(want[k - 1]) if k else "the initial state"
    return (f"{len(bad)} symbols differ, first at {k}: got {hx(got[k])} = {got[k]}, want {hx(want[k])} = {want[k]}, "
            f"state before {prev}")


# ------------------------------------------------- numpy float32 restatement ----
def np_mod_trig(x):
    """util.rs:3-6: x - TWO_PI * floor(x / TWO_PI), an IEEE f32 division, every op rounded to f32."""
    return F(x - F(TWO_PI * np.floor(F(x / TWO_PI))))


def np_mod_trig_no_correction(x):
    """A plausible wrong form: the floor of x * fl(1 / TWO_PI) without the fma correction."""
    return F(x - F(TWO_PI * np.floor(F(x * RC))))


def np_add(phase, sym, shift):
    """dmpsk.rs:31: phase + sym * shift, the product rounded before the sum."""
    return F(phase + F(sym * shift))


def np_add_fused(phase, sym, shift):
    """The same contracted to one fma: the exact product (f64 holds it) added, one rounding."""
    return F(np.float64(phase) + np.float64(sym) * np.float64(shift))


def np_sample_freq(hz, sr):
    """freq.rs:19-26: 2.0 * PI * hz as f32, divided by sr as f32."""
    pi = np.uint32(0x40490FDB).view(np.float32)
    return F(F(F(F(2.0) * pi) * F(hz)) / F(sr))


def np_states(o, spec, bits, s0, sps=SPS, mod_trig=np_mod_trig, add=np_add):
    """dmpsk.rs:29-33, mfsk.rs:68-75, bfsk.rs:42-53 in numpy float32, each operation rounded to
    f32 in the reference's order; nothing here comes from the oracle (`o` is unused)."""
    bps = bps_of(spec)
    n = len(bits) // bps
    idx = bits[:n * bps].reshape(n, bps).astype(np.int64) @ (1 << np.arange(bps)[::-1])    # MSB first
    out = np.zeros((n, 2), F)
    if spec[0] == "dmpsk":
        phase, shift = F(spec[3]), F(spec[4])
        for m in range(n):
            phase = mod_trig(add(phase, F(idx[m]), shift))
            out[m, 0] = phase
    elif spec[0] == "mfsk":
        freq, inc, mx = np_sample_freq(*spec[2]), spec[4], (1 << bps) - 1
        cur, off = F(0.0), F(0.0)
        for m in range(n):
            s = F(s0 + m * sps + 1)                           # `s as f32`
            nxt = F(2 * int(idx[m])) if inc else F(2 * int(idx[m]) - mx)
            off = F(off + F(F(F(cur - nxt) * freq) * s))
            off = mod_trig(off)
            cur = nxt
            out[m] = (cur, off)
    else:
        freq = np_sample_freq(*spec[1])
        phase, prev = F(0.0), 0
        for m in range(n):
            b, s = int(idx[m]), s0 + m * sps + 1
            if b != prev:
                d = -F(freq * F(s)) if b == 1 else F(freq * F(s - 1))
                phase = mod_trig(F(phase + d))
                prev = b
            out[m] = (phase, prev)
    return out
