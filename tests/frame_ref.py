"""Restatement of the frame synchronizer of include/modem_hip.h ("Frame synchronizer"), for the
tests: float64 for the correlation, the energy and the metric (steps 1-4), Python integers for the
positions and the rotation index, the streaming rule and the flush (step 5), the gather. It also
bounds the f32 error of the device's m and e from the stated summation order, and classifies every
position as sure or borderline against that bound."""
import math

import numpy as np

U = 2.0 ** -24                      # unit roundoff of f32


def cplx(x):
    x = np.asarray(x)
    return x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)


def energy(u):
    """Eu as the handle forms it: a double sum over the f32 values, j ascending."""
    s = 0.0
    for re, im in np.asarray(u, np.float32).astype(np.float64):
        s += re * re + im * im
    return s


def t2_of(u, thr):
    return float(np.float32(thr * thr * energy(u)))


def _windows(v, L):
    return np.lib.stride_tricks.sliding_window_view(v, L)


def correlate(x, u):
    """Step 1 in float64 for one window: (c, e, m, S) for the positions 0 .. n - L (empty when
    n < L); S[k] = sum_j |r[k+j]| |u[j]|, what the error bound is applied to."""
    r, uu = cplx(x), cplx(u)
    L = len(uu)
    if len(r) < L:
        z = np.zeros(0)
        return z.astype(complex), z, z, z
    with np.errstate(all="ignore"):
        c = _windows(r, L) @ np.conj(uu)
        e = _windows(r.real ** 2 + r.imag ** 2, L).sum(1)
        S = _windows(np.abs(r), L) @ np.abs(uu)
        m = c.real ** 2 + c.imag ** 2
    return c, e, m, S


def bounds(c, e, m, S, L, t2):
    """(dm, dt): bounds on |m_f32 - m| and on |(t2 * e)_f32 - t2 e|.

    An accumulator of c.re (or c.im) takes ceil(L / 4) terms, two fused multiply-adds each, so at
    most n = 2 ceil(L / 4) roundings lie on its chain, and the join (a0 + a1) + (a2 + a3) adds two
    more: every product enters the result through at most n + 2 roundings. With g = (n + 2) U /
    (1 - (n + 2) U) the computed component is off by at most g * sum_j (|r.re u.re| + |r.im u.im|)
    <= g S (Cauchy-Schwarz per term), so |dc| <= sqrt(2) g S. m = fma(c.re, c.re, c.im * c.im) has
    two more roundings: dm <= 2 |c| |dc| + |dc|^2 + 2 U (|c| + |dc|)^2. The energy has the same
    chains over non-negative terms: de <= g e; the product t2 * e one more rounding."""
    n = 2 * ((L + 3) // 4) + 2
    g = n * U / (1 - n * U)
    with np.errstate(all="ignore"):
        dc = math.sqrt(2.0) * g * S
        a = np.sqrt(m)
        dm = 2 * a * dc + dc * dc + 2 * U * (a + dc) ** 2
        dt = t2 * e * (g + 2 * U)
    return dm, dt


def detect(x, u, W, thr):
    """Steps 1-4 and the flush for one window (a stream from its first symbol, or from the first
    symbol after a flush, to a flush). Returns a dict: pos (list of ints, relative to the window),
    turn (angle of c as a fraction of a turn, float64), metric, m, e, c, and `borderline`, the
    positions whose fate an f32 evaluation within the bounds could change."""
    L = len(u)
    eu, t2 = energy(u), t2_of(u, thr)
    eu32 = float(np.float32(eu))
    c, e, m, S = correlate(x, u)
    dm, dt = bounds(c, e, m, S, L, t2)
    n = len(m)
    fin = np.isfinite(m) & np.isfinite(e)
    with np.errstate(all="ignore"):
        ok = fin & (m > 0) & (m >= t2 * e)
        near = fin & (np.abs(m - t2 * e) <= dm + dt)
    pos, borderline = [], []
    for k in np.nonzero(ok | near)[0]:
        k = int(k)
        lo, hi = max(0, k - W), min(n - 1, k + W)
        before, after = m[lo:k], m[k + 1:hi + 1]
        fb, fa = np.isfinite(before), np.isfinite(after)
        hit = bool(ok[k]) and not np.any(before[fb] >= m[k]) and not np.any(after[fa] > m[k])
        nb = np.concatenate([np.arange(lo, k)[fb], np.arange(k + 1, hi + 1)[fa]])
        close = np.abs(m[nb] - m[k]) <= dm[nb] + dm[k]
        # a close comparison matters unless some sure comparison rejects k anyway
        sure_reject = np.any((before[fb] >= m[k]) & ~close[: fb.sum()]) or np.any((after[fa] > m[k]) & ~close[fb.sum():])
        if near[k] and not sure_reject:
            borderline.append(k)
        elif np.any(close) and not sure_reject:
            borderline.append(k)
        if hit:
            pos.append(k)
    p = np.array(pos, dtype=np.int64)
    with np.errstate(all="ignore"):
        metric_all = np.where(fin & (e > 0), np.sqrt(m / np.where(e > 0, e * eu32, 1.0)), 0.0)
    return dict(pos=pos, turn=(np.angle(c[p]) / (2 * np.pi)) % 1.0, metric=metric_all[p], metric_all=metric_all,
                m=m, e=e, c=c, dm=dm, borderline=borderline, t2=t2, eu=eu, L=L)


def metric_bound(res, k):
    """|metric_f32 - metric| at the hit k: the square root halves the relative errors of m (dm / m),
    of e (g, see bounds()), of the product e * Eu and of the division (U each), and rounds once
    more (U); 1 % on top for the second-order terms."""
    n = 2 * ((res["L"] + 3) // 4) + 2
    g = n * U / (1 - n * U)
    return 1.01 * res["metric_all"][k] * (0.5 * (res["dm"][k] / res["m"][k] + g + 2 * U) + U)


def decided(T, W, L):
    """Step 5: how many positions of a window are decided once it holds T symbols."""
    return max(0, T - W - L + 1)


def rot_of(phi, power):
    """The gather's rotation index from a 32-bit phi (Python integers)."""
    if power == 1:
        return 0
    lm = power.bit_length() - 1
    return ((int(phi) + (1 << (31 - lm))) & 0xFFFFFFFF) >> (32 - lm)


def gather(x, base, pos, phi, count, skip, length, power):
    """(frames (cap, length) complex128, ok (cap,) uint8) of the gather; phi None: no rotation."""
    r = cplx(x)
    cap = len(pos)
    out = np.zeros((cap, length), dtype=np.complex128)
    ok = np.zeros(cap, dtype=np.uint8)
    for f in range(min(int(count), cap)):
        a = int(pos[f]) + skip - base
        if a < 0 or a + length > len(r):
            continue
        rot = 0 if phi is None else rot_of(phi[f], power)
        out[f] = r[a:a + length] * np.exp(-2j * np.pi * rot / power)
        ok[f] = 1
    return out, ok


def turn_dist(phi, turn):
    """Distance in turns between 32-bit phis and float64 turns, mod 1."""
    d = np.asarray(phi, np.float64) / 2.0 ** 32 - np.asarray(turn, np.float64)
    return np.abs(d - np.round(d))


# ------------------------------------------------ the noisy cases of the two test files ----
# name: (constellation, L, float16 input, log2 gain, phase, seed). A stream of 1500 random symbols
# with the unique word at three places, AWGN of sigma 0.25 per symbol (relative to unit-rms points);
# W = L, thr = 0.6. tests/test_frame_host.py proves every one free of borderline positions.
NOISY = {
    "qpsk-32-f32": ("qpsk", 32, False, -10, 0.7, 11),
    "qpsk-64-f16": ("qpsk", 64, True, 10, 2.9, 12),
    "qam16-32-f16": ("qam16", 32, True, -3, 4.4, 13),
    "qam16-64-f32": ("qam16", 64, False, 7, 5.9, 14),
}
NOISY_STARTS = (5, 517, 1023)
NOISY_THR = 0.6


def noisy_case(m, name):
    """(x (1500, 2) float32 or float16, u (L, 2) float32) of a NOISY case."""
    kind, L, half, lg, phase, seed = NOISY[name]
    lut = (m.QPSK(0.0, 1.0) if kind == "qpsk" else m.QAM(4, 0.0, 1.0)).lut()
    t = cplx(lut)
    rms = math.sqrt(float(np.mean(np.abs(t) ** 2)))
    rng = np.random.RandomState(seed)
    uw = rng.randint(0, len(t), L)
    sym = rng.randint(0, len(t), 1500)
    for s in NOISY_STARTS:
        sym[s:s + L] = uw
    w = (rng.standard_normal(1500) + 1j * rng.standard_normal(1500)) * (0.25 * rms / math.sqrt(2.0))
    z = (t[sym] + w) * (2.0 ** lg) * np.exp(1j * phase)
    x = np.stack([z.real, z.imag], 1).astype(np.float16 if half else np.float32)
    return x, lut[uw]


# ------------------------------------------------- the loopback of the two test files ----
# 64 frames of a 64-symbol unique word and 448 payload symbols, a gap of 0..99 random symbols
# before each, through a 65-tap RRC at sps 4, the channel's offset and a phase a quarter turn past
# what phase0 = 0 resolves: the conditions of tests/test_gpu_frame_loopback.py, confirmed on the
# oracle's chain in tests/test_frame_host.py.
LOOP = dict(sps=4, L=65, frames=64, uw=64, payload=448, cfo=1e-4, phase=0.3 + math.pi / 2, block=256, guard=64,
            threshold=0.6, uw_seed=0xF4A3E, bits_seed=0xC4A2, gap_seed=77, noise_seed=2024,
            qpsk_ebn0_db=8.0, qam_ebn0_db=12.0, tail=128)


def loop_stream(prng_bits, bps):
    """(bits uint8, starts: the symbol index of each unique word, uw symbols (64,) ints). The stream
    ends with LOOP['tail'] random symbols, so that the last frame's payload is followed by more
    than guard + uw symbols and is decided without a flush."""
    C = LOOP
    gaps = np.random.RandomState(C["gap_seed"]).randint(0, 100, C["frames"])
    per = C["uw"] + C["payload"]
    nsym = int(gaps.sum()) + C["frames"] * per + C["tail"]
    nsym = (nsym + C["block"] - 1) // C["block"] * C["block"]     # whole blocks of the carrier synchronizer
    bits = np.array(prng_bits(C["bits_seed"], nsym * bps), dtype=np.uint8)
    uwb = np.array(prng_bits(C["uw_seed"], C["uw"] * bps), dtype=np.uint8)
    starts, k = [], 0
    for g in gaps:
        k += int(g)
        bits[k * bps:(k + C["uw"]) * bps] = uwb
        starts.append(k)
        k += per
    uw = uwb.reshape(-1, bps).astype(np.int64) @ (1 << np.arange(bps)[::-1])
    return bits, starts, uw


def payload_bits(bits, starts, bps):
    """(frames, payload * bps) uint8: the payload bits sent."""
    C = LOOP
    return np.stack([bits[(s + C["uw"]) * bps:(s + C["uw"] + C["payload"]) * bps] for s in starts])
