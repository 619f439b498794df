"""Restatement of the carrier synchronizer of include/modem_hip.h ("Carrier synchronizer"), for the
tests: float64 for the block sums, the quality and the angle (steps 1-2), Python integers for the
unwrap and the phase line (steps 3-4), float64 for the rotation. The uint64 turns of `ref_phase`
and `phase0` are taken from the product's own conversion (`Channel.nco`, checked against an exact
evaluation in tests/test_chan_host.py), not restated here."""
import numpy as np

MASK = (1 << 64) - 1
BAD_DEVICE = 1 << 20


def turns(m, v):
    """frac(v / 2 pi) * 2^64 as modem_chan_create forms phase0 (no device needed)."""
    return m.Channel(phase=float(v), device=BAD_DEVICE).nco[1]


def sext(v):
    v &= MASK
    return v - (1 << 64) if v >> 63 else v


def cplx(x):
    x = np.asarray(x)
    return x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)


def estimates(x, power, block, norm, ref):
    """Steps 1-2 for the whole blocks of the (n, 2) symbols x (any float dtype, widened exactly;
    norm enters as the f32 the handle holds). Returns (q float64 (nb,), turn float64 (nb,): the
    angle of P_b as a fraction of a turn in [0, 1), Phi: list of ints, turn rounded to 32 bits)."""
    r = cplx(x)
    nb = len(r) // block
    z = (float(np.float32(norm)) * r[: nb * block].reshape(nb, block)) ** power
    P, S = z.sum(1), np.abs(z).sum(1)
    ok = np.isfinite(P) & np.isfinite(S) & (S > 0)
    q = np.where(ok, np.abs(P) / np.where(ok, S, 1.0), 0.0)
    turn = np.where(np.isfinite(P) & (P != 0), np.angle(P) / (2 * np.pi), 0.0) % 1.0
    Phi = [(((int(round(t * 2.0 ** 32)) & 0xFFFFFFFF) << 32) - ref) & MASK for t in turn]
    return q, turn, Phi


def unwrap(Phi, power, phase0):
    """Step 3: theta_b for the Phi_b (ints), and each block's unwrap margin 0.5 - |wrap(Phi_b - Phi_{b-1})| in turns."""
    lm = power.bit_length() - 1
    theta, margins = [], []
    th, prev = phase0 & MASK, (power * phase0) & MASK
    for p in Phi:
        d = sext(p - prev)
        th = (th + (d >> lm)) & MASK
        theta.append(th)
        margins.append(0.5 - abs(d) / 2.0 ** 64)
        prev = p
    return theta, margins


def phases(theta, block, phase0, flat=False, nflush=0):
    """Step 4: ph of every symbol of the blocks (ints), then of `nflush` flushed symbols."""
    lb = block.bit_length() - 1
    ph, prev, s, th = [], None, 0, phase0 & MASK
    for th in theta:
        d = 0 if prev is None else sext(th - prev)
        s = 0 if flat else d >> (lb + 1)
        ph += [(th + s * (2 * i - block + 1)) & MASK for i in range(block)]
        prev = th
    ph += [(th + s * (2 * (i + block) - block + 1)) & MASK for i in range(nflush)]
    return ph


def derotate(x, ph):
    """x e^{-j 2 pi ph / 2^64} for the (n, 2) symbols x, from the top 53 bits of each phase. (n, 2) float64."""
    a = np.array([p >> 11 for p in ph], dtype=np.float64) * 2.0 ** -53
    y = cplx(x) * np.exp(-2j * np.pi * a)
    return np.stack([y.real, y.imag], 1)


def top32(ph):
    """The phases the device rotates by: the top 32 bits, the rest cleared."""
    return [p & ~0xFFFFFFFF for p in ph]


def sync(x, power, block, norm, ref, phase0, flat=False):
    """The whole chain on one stream, flush included. Returns a dict: out (n, 2) float64, theta (ints),
    q, turn, Phi, margins."""
    q, turn, Phi = estimates(x, power, block, norm, ref)
    theta, margins = unwrap(Phi, power, phase0)
    n = len(x)
    ph = phases(theta, block, phase0, flat, n - len(theta) * block)
    return dict(out=derotate(x, ph), theta=theta, q=q, turn=turn, Phi=Phi, margins=margins, ph=ph)


# ------------------------------------------------- the same steps for millions of symbols ----
# numpy uint64 / int64 wrap-around arithmetic in place of the Python integers, a cumsum in place of
# the recurrences. tests/test_sync_host.py holds every one equal to the function above it, element
# for element; that equality is what lets tests/test_gpu_second_trip.py use them.
def _u64(v):
    return np.asarray(v, dtype=np.uint64)


def estimates_np(x, power, block, norm, ref):
    """estimates() with Phi as a uint64 array."""
    r = cplx(x)
    nb = len(r) // block
    z = (float(np.float32(norm)) * r[: nb * block].reshape(nb, block)) ** power
    P, S = z.sum(1), np.abs(z).sum(1)
    ok = np.isfinite(P) & np.isfinite(S) & (S > 0)
    q = np.where(ok, np.abs(P) / np.where(ok, S, 1.0), 0.0)
    turn = np.where(np.isfinite(P) & (P != 0), np.angle(P) / (2 * np.pi), 0.0) % 1.0
    t32 = (np.rint(turn * 2.0 ** 32).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    return q, turn, (t32 << np.uint64(32)) - np.uint64(ref & MASK)


def unwrap_np(Phi, power, phase0):
    """unwrap() on a uint64 array: (theta uint64 (nb,), margins float64 (nb,))."""
    Phi = _u64(Phi)
    lm = power.bit_length() - 1
    prev = np.concatenate([_u64([(power * phase0) & MASK]), Phi])[: len(Phi)]
    d = (Phi - prev).view(np.int64)
    theta = np.uint64(phase0 & MASK) + np.cumsum((d >> lm).view(np.uint64), dtype=np.uint64)
    return theta, 0.5 - np.abs(d.astype(np.float64)) / 2.0 ** 64


def phases_np(theta, block, phase0, flat=False, nflush=0):
    """phases() on a uint64 array of theta: uint64 (nb * block + nflush,)."""
    theta = _u64(theta)
    lb = block.bit_length() - 1
    d = np.zeros(len(theta), np.int64)
    d[1:] = (theta[1:] - theta[:-1]).view(np.int64)
    s = np.zeros_like(d) if flat else d >> (lb + 1)
    i = 2 * np.arange(block, dtype=np.int64) - block + 1
    ph = (theta[:, None] + (s[:, None] * i[None, :]).view(np.uint64)).reshape(-1)
    th, sl = (theta[-1], s[-1]) if len(theta) else (np.uint64(phase0 & MASK), np.int64(0))
    f = 2 * (np.arange(nflush, dtype=np.int64) + block) - block + 1
    return np.concatenate([ph, th + (sl * f).view(np.uint64)])


def derotate_np(x, ph):
    """derotate() on a uint64 array of phases."""
    a = (_u64(ph) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    y = cplx(x) * np.exp(-2j * np.pi * a)
    return np.stack([y.real, y.imag], 1)


def top32_np(ph):
    return _u64(ph) & np.uint64(0xFFFFFFFF00000000)


def sync_np(x, power, block, norm, ref, phase0, flat=False):
    """sync() from the variants above: arrays where sync() has lists."""
    q, turn, Phi = estimates_np(x, power, block, norm, ref)
    theta, margins = unwrap_np(Phi, power, phase0)
    ph = phases_np(theta, block, phase0, flat, len(x) - len(theta) * block)
    return dict(out=derotate_np(x, ph), theta=theta, q=q, turn=turn, Phi=Phi, margins=margins, ph=ph)


# ------------------------------------------------- the loopback of the two test files ----
# QPSK(0, 1) / QAM16 through a 65-tap RRC at sps 4, the channel's offset and phase, 2^17 bits: the
# conditions of tests/test_gpu_sync_loopback.py, confirmed on the oracle's chain in
# tests/test_sync_host.py.
LOOP = dict(sps=4, L=65, nbits=1 << 17, cfo=1e-4, phase=0.3, block=256, bits_seed=0xC4A2, noise_seed=2024,
            qpsk_ebn0_db=8.0, qam_ebn0_db=12.0)


def loop_n0(lut, ebn0_db):
    """n0 for Eb/N0 with unit-energy matched taps: Eb = mean |lut|^2 / bps (include/modem_hip.h)."""
    lut = np.asarray(lut, np.float64)
    bps = int(lut.shape[0]).bit_length() - 1
    return float(np.mean(np.sum(lut ** 2, 1))) / (bps * 10.0 ** (ebn0_db / 10))


def ber_band(nbits, ebn0_db):
    """(expected bit errors, 5 binomial sigmas) of QPSK at Eb/N0."""
    import math
    p = 0.5 * math.erfc(math.sqrt(10.0 ** (ebn0_db / 10)))
    return nbits * p, 5 * math.sqrt(nbits * p * (1 - p))


def loop_true_phase(k):
    """The channel's phase, in turns, at the sample that carries symbol k (its matched-filter peak:
    sample sps k + L - 1 of the channel's stream)."""
    return (LOOP["phase"] + LOOP["cfo"] * (LOOP["sps"] * np.asarray(k, np.float64) + LOOP["L"] - 1)) / (2 * np.pi)


def slips(theta, block):
    """Worst distance, in turns, of theta_b from the true phase at the block centres."""
    kc = np.arange(len(theta)) * block + (block - 1) / 2
    d = np.array([t / 2.0 ** 64 for t in theta]) - loop_true_phase(kc)
    return float(np.abs(d - np.round(d)).max()) if len(theta) else 0.0
