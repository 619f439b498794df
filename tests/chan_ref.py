"""Float64 restatement of the channel model of include/modem_hip.h ("Channel model"), for the
tests: the counter-based Gaussian, the NCO rotation from its exact integer phases, and the channel
itself. numpy uint64 wrap-around arithmetic for the generator, Python ints for the phases. The NCO
integers are taken from `Channel.nco` by the callers, not restated here."""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def mix(z):
    """splitmix64's finaliser on a uint64 array."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def words(seed, n0_index, n):
    """word[i] for the absolute sample indices n0_index .. n0_index + n - 1."""
    k = int(mix(np.array([(int(seed) + GOLDEN) & MASK], dtype=np.uint64))[0])
    idx = (np.arange(n, dtype=np.uint64) + np.uint64(int(n0_index) & MASK))
    with np.errstate(over="ignore"):
        return mix(np.uint64(k) + (idx + np.uint64(1)) * np.uint64(GOLDEN))


def noise_parts(seed, n0_index, n):
    """(r, u2): r = sqrt(-ln u1) and the turn fraction u2, float64."""
    w = words(seed, n0_index, n)
    u1 = ((w >> np.uint64(40)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = ((w & np.uint64(0xFFFFFFFF)) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-np.log(u1)), u2


def noise(seed, n0_index, n):
    """w[n0_index .. n0_index + n - 1], complex128, E|w|^2 = 1."""
    r, u2 = noise_parts(seed, n0_index, n)
    return r * np.exp(2j * np.pi * u2)


def rotate(step, phase0, n_index, n):
    """e^{j theta} for the absolute indices n_index .. n_index + n - 1: the exact 64-bit phase as
    a Python int, its top 53 bits as a float64 fraction of a turn (error < 2^-53 turns)."""
    ph = [((phase0 + step * (n_index + i)) & MASK) >> 11 for i in range(n)]
    return np.exp(2j * np.pi * (np.array(ph, dtype=np.float64) * 2.0 ** -53))


def rotate_np(step, phase0, n_index, n):
    """rotate() in numpy uint64 wrap-around arithmetic, for millions of samples
    (tests/test_chan_host.py holds it equal to rotate(), element for element)."""
    with np.errstate(over="ignore"):
        idx = np.arange(n, dtype=np.uint64) + np.uint64(int(n_index) & MASK)
        ph = (np.uint64(int(phase0) & MASK) + np.uint64(int(step) & MASK) * idx) >> np.uint64(11)
    return np.exp(2j * np.pi * (ph.astype(np.float64) * 2.0 ** -53))


def channel(x, gain=1.0, nco=(0, 0), n0=0.0, seed=0, s0=0, rotate=rotate):
    """y for the (n, 2) samples x (any float dtype, widened exactly). gain and sqrt(n0) enter as
    the f32 values the handle holds. Returns (y (n, 2) float64, r (n,): sqrt(-ln u1), or zeros).
    `rotate`: rotate, or rotate_np for long streams."""
    x = np.asarray(x)
    n = x.shape[0]
    xc = x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)
    step, phase0 = nco
    y = float(np.float32(gain)) * xc
    if step or phase0:
        y = y * rotate(step, phase0, int(s0), n)
    r = np.zeros(n)
    if n0:
        r, u2 = noise_parts(seed, s0, n)
        y = y + float(np.float32(np.sqrt(n0))) * r * np.exp(2j * np.pi * u2)
    return np.stack([y.real, y.imag], 1), r
