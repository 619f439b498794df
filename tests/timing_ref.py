"""Restatement of the symbol timing synchronizer of include/modem_hip.h ("Symbol timing
synchronizer"), for the tests: float64 for the phase energies, the line, the quality and the angle
(steps 1-2), integers for the unwrap, the line and Q, m, mu (steps 3-4; numpy int64, every value is
below 2^50), float64 for the interpolation. And a float64 stream generator: symbols through a
raised-cosine pulse evaluated directly at the sample instants, so that a delay and a drift need no
resampler."""
import math

import numpy as np

BAD_DEVICE = 1 << 20
ONE = 1 << 32


def cplx(x):
    x = np.asarray(x)
    return x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)


def pairs(z):
    return np.stack([z.real, z.imag], 1)


# ------------------------------------------------------------------ the generator ----
def rc(t, beta):
    """The raised-cosine pulse (T = 1) at the float64 times t."""
    t = np.asarray(t, np.float64)
    den = 1.0 - (2.0 * beta * t) ** 2
    sing = np.abs(den) < 1e-9
    out = np.sinc(t) * np.cos(np.pi * beta * t) / np.where(sing, 1.0, den)
    return np.where(sing, np.pi / 4 * np.sinc(1.0 / (2.0 * beta)) if beta > 0 else 1.0, out)


def stream(points, sps, n, tau, drift=0.0, beta=0.5, reach=10):
    """n samples x[j] = sum_k points[k] rc(t_j - k), t_j = j / sps - (tau + drift * j / sps): the
    centre of the eye of symbol k lags the grid instant k * sps by tau + drift * k symbols (to first
    order in drift). points: complex symbols, indexed from 0, zero outside. complex128 (n,)."""
    j = np.arange(n, dtype=np.float64) / sps
    t = j - (tau + drift * j)
    k0 = np.floor(t).astype(np.int64)
    x = np.zeros(n, np.complex128)
    pts = np.asarray(points, np.complex128)
    for dk in range(-reach, reach + 1):
        k = k0 + dk
        ok = (k >= 0) & (k < len(pts))
        x += np.where(ok, pts[np.clip(k, 0, len(pts) - 1)], 0.0) * rc(t - k, beta)
    return x


def true_delay(k, tau, drift):
    """The delay, in symbols, at grid symbol k."""
    return tau + drift * np.asarray(k, np.float64)


# ------------------------------------------------------------------ steps 1 - 4 ----
def estimates(x, sps, block):
    """Steps 1-2 for the whole blocks of the complex samples x. Returns (q, turn, Phi): q float64
    (nb,), turn float64 (nb,) = Phi_b / 2^32 in [0, 1) before rounding, Phi list of ints."""
    nb = len(x) // (block * sps)
    e = (np.abs(x[: nb * block * sps]) ** 2).reshape(nb, block, sps).sum(1)
    S = e.sum(1)
    X = (e * np.exp(-2j * np.pi * np.arange(sps) / sps)).sum(1)
    ok = np.isfinite(X) & np.isfinite(S) & (S > 0)
    q = np.where(ok, np.abs(X) / np.where(ok, S, 1.0), 0.0)
    turn = np.where(np.isfinite(X) & (X != 0), -np.angle(X) / (2 * np.pi), 0.0) % 1.0
    Phi = [int(round(t * 2.0 ** 32)) & 0xFFFFFFFF for t in turn]
    return q, turn, Phi


def sext32(v):
    v &= 0xFFFFFFFF
    return v - ONE if v >> 31 else v


def d_start(tau0):
    return int(np.rint(tau0 * 2.0 ** 32))


def unwrap(Phi, D_start):
    """Step 3: D_b for the Phi_b (ints), and each block's unwrap margin 0.5 - |wrap| / 2^32 in symbols."""
    D, margins, cur = [], [], int(D_start)
    for p in Phi:
        w = sext32(int(p) - cur)
        cur += w
        D.append(cur)
        margins.append(0.5 - abs(w) / 2.0 ** 32)
    return D, margins


def positions(D, D_start, sps, block, span, flat=False, nflush=0, first=True):
    """Step 4: (m, mu24) of every output of the blocks with delays D (ints), then of `nflush`
    flushed symbols; m counts samples from the first sample of the first block, mu24 = mu * 2^24.
    `first`: D[0] is the stream's first block (s = 0)."""
    lb = block.bit_length() - 1
    i = np.arange(block, dtype=np.int64)
    ms, mus, prev, s, cur = [], [], None, 0, int(D_start)
    lim = span * ONE

    def place(cur, s, line_i, out_i, base):
        e = np.clip(cur + s * (2 * line_i - block + 1), -lim, lim)
        Q = sps * ((out_i - span) * ONE + e)
        ms.append(base + (Q >> 32))
        mus.append((Q & 0xFFFFFFFF) >> 8)

    for b, cur in enumerate(D):
        d = 0 if (prev is None and first) else cur - (int(D_start) if prev is None else prev)
        s = 0 if flat else d >> (lb + 1)
        place(cur, s, i, i, b * block * sps)
        prev = cur
    if nflush:
        f = np.arange(nflush, dtype=np.int64)
        place(cur, s, f + block, f, len(D) * block * sps)
    if not ms:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(ms), np.concatenate(mus)


def coefs(mu):
    return np.stack([-mu * (mu - 1) * (mu - 2) / 6, (mu + 1) * (mu - 1) * (mu - 2) / 2,
                     -(mu + 1) * mu * (mu - 2) / 2, (mu + 1) * mu * (mu - 1) / 6], 1)


def taps_of(x, m):
    """The four samples x[m - 1 .. m + 2] of every position, zeros outside x. (len(m), 4) complex."""
    idx = m[:, None] + np.arange(-1, 3)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    return np.where(ok, x[np.clip(idx, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0)


def interpolate(x, m, mu24):
    """out and the four taps of every position, in float64."""
    t = taps_of(x, m)
    return (coefs(mu24.astype(np.float64) * 2.0 ** -24) * t).sum(1), t


def timing(x, sps, block, span, tau0, flat=False):
    """The whole chain on one stream of complex samples, flush included. Returns a dict."""
    q, turn, Phi = estimates(x, sps, block)
    D, margins = unwrap(Phi, d_start(tau0))
    nflush = (len(x) - len(D) * block * sps) // sps
    m, mu24 = positions(D, d_start(tau0), sps, block, span, flat, nflush)
    out, taps = interpolate(x, m, mu24)
    return dict(out=out, taps=taps, D=D, q=q, turn=turn, Phi=Phi, margins=margins, m=m, mu24=mu24)


# ------------------------------------------------- the same steps for millions of samples ----
# int64 arrays and a cumsum in place of the per-block Python loops. tests/test_timing_host.py holds
# every one equal to the function above it, element for element; that equality is what lets
# tests/test_gpu_second_trip.py use them.
def estimates_np(x, sps, block):
    """estimates() with Phi as an int64 array."""
    nb = len(x) // (block * sps)
    e = (np.abs(x[: nb * block * sps]) ** 2).reshape(nb, block, sps).sum(1)
    S = e.sum(1)
    X = (e * np.exp(-2j * np.pi * np.arange(sps) / sps)).sum(1)
    ok = np.isfinite(X) & np.isfinite(S) & (S > 0)
    q = np.where(ok, np.abs(X) / np.where(ok, S, 1.0), 0.0)
    turn = np.where(np.isfinite(X) & (X != 0), -np.angle(X) / (2 * np.pi), 0.0) % 1.0
    return q, turn, np.rint(turn * 2.0 ** 32).astype(np.int64) & 0xFFFFFFFF


def unwrap_np(Phi, D_start):
    """unwrap() on an array: (D int64 (nb,), margins float64 (nb,)). D_b - D_start is the running
    sum of the wraps w_b, and w_b = sext32(Phi_b - D_{b-1}) depends only on the low 32 bits of
    D_{b-1}, which are Phi_{b-1}: w_b = sext32(Phi_b - Phi_{b-1})."""
    Phi = np.asarray(Phi, dtype=np.int64)
    prev = np.concatenate([np.array([int(D_start)], np.int64), Phi])[: len(Phi)]
    w = ((Phi - prev) & 0xFFFFFFFF)
    w = w - ((w >> 31) << 32)
    return int(D_start) + np.cumsum(w), 0.5 - np.abs(w) / 2.0 ** 32


def positions_np(D, D_start, sps, block, span, flat=False, nflush=0, first=True):
    """positions() on an int64 array of D."""
    D = np.asarray(D, dtype=np.int64)
    lb = block.bit_length() - 1
    lim = span * ONE
    prev = np.concatenate([np.array([int(D_start)], np.int64), D])[: len(D)]
    d = D - prev
    if first and len(d):
        d[0] = 0
    s = np.zeros_like(d) if flat else d >> (lb + 1)
    i = np.arange(block, dtype=np.int64)
    e = np.clip(D[:, None] + s[:, None] * (2 * i - block + 1)[None, :], -lim, lim)
    Q = sps * ((i[None, :] - span) * ONE + e)
    ms = (np.arange(len(D), dtype=np.int64) * (block * sps))[:, None] + (Q >> 32)
    ms, mus = ms.reshape(-1), ((Q & 0xFFFFFFFF) >> 8).reshape(-1)
    if nflush:
        cur, sl = (int(D[-1]), int(s[-1])) if len(D) else (int(D_start), 0)
        f = np.arange(nflush, dtype=np.int64)
        e = np.clip(cur + sl * (2 * (f + block) - block + 1), -lim, lim)
        Q = sps * ((f - span) * ONE + e)
        ms = np.concatenate([ms, len(D) * block * sps + (Q >> 32)])
        mus = np.concatenate([mus, (Q & 0xFFFFFFFF) >> 8])
    return ms, mus


def timing_np(x, sps, block, span, tau0, flat=False):
    """timing() from the variants above: arrays where timing() has lists."""
    q, turn, Phi = estimates_np(x, sps, block)
    D, margins = unwrap_np(Phi, d_start(tau0))
    nflush = (len(x) - len(D) * block * sps) // sps
    m, mu24 = positions_np(D, d_start(tau0), sps, block, span, flat, nflush)
    out, taps = interpolate(x, m, mu24)
    return dict(out=out, taps=taps, D=D, q=q, turn=turn, Phi=Phi, margins=margins, m=m, mu24=mu24)


# ------------------------------------------------------------------ the bounds ----
U = 2.0 ** -24


def line_c(sps, block):
    """|X_dev - X| <= c u S_b (tests/test_gpu_timing.py derives it): 2 for fma(re, re, im*im), the
    serial adds of an accumulator (B N / 512, at least 1), 2 for the join of the four, the tree
    levels (4, and 5 when N = 4), 1 for a difference of two E_p, and 4 more when N = 8 (the rounded
    h, its product, the inner and the outer sum)."""
    return 2 + max(1, block * sps // 512) + 2 + (5 if sps == 4 else 4) + 1 + (4 if sps == 8 else 0)


def phi_bound(q, sps, block):
    """symbols: the angle of a vector of length |X| moved by c u S, plus turn32's own bound."""
    return (line_c(sps, block) * U / q) / (2 * np.pi) + 2.0 ** -22


def q_bound(sps, block):
    """|X| moved by c u S and rounded 4 times (quotient, fma, square root, product), S by the
    summation part of c, the division once: (2 c + 6) u, for q <= 1."""
    return (2 * line_c(sps, block) + 6) * U


OUT_C = 12     # out within 12 u max|tap| (tests/test_gpu_timing.py derives it)


# ------------------------------------------------- the loopback of the two test files ----
# QPSK(0, 1) / QAM16 through a 65-tap RRC at sps 4 whose TX taps are sampled 1.3 samples late, the
# channel's offset, phase and noise, 2^17 bits: the conditions of tests/test_gpu_timing_loopback.py,
# computed on the oracle's chain in tests/test_timing_host.py.
LOOP = dict(sps=4, L=65, beta=0.35, nbits=1 << 17, offset=1.3, cfo=1e-4, phase=0.3, tblock=1024, span=2, block=256,
            bits_seed=0xC4A2, noise_seed=2024, qpsk_ebn0_db=8.0, qam_ebn0_db=12.0,
            skip_blocks=1,        # timing blocks whose symbols are not counted: the start-up transient
            qpsk_errors=28,       # bit errors of the restatements on the oracle's chain (test_timing_host.py)
            tau_margin=0.05)       # symbols: the bound on |tau_b - 0.325| for QAM16 at 12 dB, B = 1024


def loop_lag():
    """Output symbol k + lag carries sent symbol k: (L - 1) / sps symbols of the two filters, span of the synchronizer."""
    return (LOOP["L"] - 1) // LOOP["sps"] + LOOP["span"]


def binomial_band(nbits, errors):
    p = errors / nbits
    return 5 * math.sqrt(nbits * p * (1 - p))


# ------------------------------------------------- the streams of tests/test_gpu_timing.py ----
# name: (sps, block, samples). QPSK symbols through the raised cosine (roll-off 0.5), the delay
# 0.3 symbol at the start and drifting by 0.2 symbol per block, white noise at Eb/N0 = 12 dB; the
# tracker starts 0.1 symbol away from the true delay.
CASES = {
    "n4_b32": (4, 32, 5 * 32 * 4 + 17),
    "n4_b256": (4, 256, 3 * 256 * 4 + 1),
    "n8_b64": (8, 64, 4 * 64 * 8),
    "n4_b4096": (4, 4096, 2 * 4096 * 4 + 5),
}
CASE_TAU, CASE_DRIFT, CASE_TAU0, CASE_SPAN, CASE_BETA, CASE_EBN0_DB = 0.3, 0.2, 0.4, 2, 0.5, 12.0
_CASE_STREAMS = {}


def case_stream(name, sps=None, block=None, n=None):
    """(x float32 (n, 2), sps, block): computed once per case and shared, never modified."""
    s0, b0, n0 = CASES[name]
    sps, block, n = sps or s0, block or b0, n or n0
    key = (name, sps, block, n)
    if key not in _CASE_STREAMS:
        rng = np.random.RandomState(len(name) * 1000 + block + sps)
        nsym = n // sps + 2
        pts = ((2 * rng.randint(0, 2, nsym) - 1) + 1j * (2 * rng.randint(0, 2, nsym) - 1)) / np.sqrt(2)
        z = stream(pts, sps, n, CASE_TAU, CASE_DRIFT / block, CASE_BETA)
        sig = np.sqrt(1.0 / (2 * 10.0 ** (CASE_EBN0_DB / 10)) / 2)        # n0 = Es / (2 Eb/N0), Es = 1
        z = z + sig * (rng.randn(n) + 1j * rng.randn(n))
        x = pairs(z).astype(np.float32)
        x.setflags(write=False)
        _CASE_STREAMS[key] = (x, sps, block)
    return _CASE_STREAMS[key]
