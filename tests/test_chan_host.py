"""Channel model, host side (no device needed): the C ABI entry points exist and refuse bad
arguments before they look for a device; the NCO integers against an exact evaluation of
frac(cfo / 2 pi); the statistics of the counter-based Gaussian of tests/chan_ref.py (the float64
restatement the GPU tests compare the kernel with); and the oracle's QPSK loopback around that
restatement, whose bit-error count must sit in the band the GPU loopback test uses."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import chan_ref

BAD_DEVICE = 1 << 20
SYMBOLS = ("modem_chan_create", "modem_chan_process", "modem_chan_set_n0", "modem_chan_nco", "modem_chan_sample",
           "modem_chan_destroy", "modem_count_errors")
# pi to about 1390 bits (Machin), as a fraction: frac(cfo / 2 pi) of every test value to 2^-300
_ONE = 1 << 1400


def _atan_inv(q):
    t = s = _ONE // q
    k, sign = 1, -1
    while t:
        t //= q * q
        k += 2
        s += sign * (t // k)
        sign = -sign
    return s


PI = Fraction(16 * _atan_inv(5) - 4 * _atan_inv(239), _ONE)


def _create(m, gain=1.0, phase=0.0, cfo=0.0, n0=0.0, seed=0, s0=0, in_dtype=0, out_dtype=0, device=0, out="handle"):
    h = ctypes.c_void_p(0xDEAD)
    st = m.load_library().modem_chan_create(gain, phase, cfo, n0, seed, s0, in_dtype, out_dtype, device,
                                            None if out is None else ctypes.byref(h))
    return st, h


def test_library_exports_the_channel(m):
    lib = ctypes.CDLL(m.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert m.load_library().modem_abi_version() == 6      # additive: the version stays
    for name in ("Channel", "count_errors"):
        assert name in m.__all__ and hasattr(m, name)


@pytest.mark.parametrize("device", [0, BAD_DEVICE])
def test_create_refusals_come_before_the_device(m, device):
    inf, nan = float("inf"), float("nan")
    bad = [dict(gain=inf), dict(gain=nan), dict(phase=-inf), dict(phase=nan), dict(cfo=inf), dict(cfo=nan),
           dict(n0=-1e-30), dict(n0=nan), dict(n0=inf), dict(n0=-inf),
           dict(in_dtype=m.DTYPE_I16), dict(in_dtype=m.DTYPE_I8), dict(out_dtype=m.DTYPE_I16), dict(out_dtype=m.DTYPE_I8),
           dict(in_dtype=-1), dict(out_dtype=4)]
    for kw in bad:
        st, h = _create(m, device=device, **kw)
        assert st == m.ERR_INVALID_ARG, kw
        assert h.value is None, kw
    st, _ = _create(m, device=device, out=None)
    assert st == m.ERR_INVALID_ARG
    st, h = _create(m, device=-1)
    assert st == m.ERR_NO_DEVICE and h.value is None
    for kw in (dict(gain=float("inf")), dict(n0=-1.0), dict(in_dtype=m.DTYPE_I8), dict(cfo=float("nan"))):
        with pytest.raises(m.ModemPanic):
            m.Channel(device=device, **kw)


def test_process_refusals_come_before_the_device(m):
    L = m.load_library()
    x = np.zeros((8, 2), np.float32)
    y = np.zeros((8, 2), np.float32)
    assert L.modem_chan_process(None, x.ctypes.data, 1, y.ctypes.data, 8, None) == m.ERR_INVALID_ARG
    assert L.modem_chan_destroy(None) == m.MODEM_OK and L.modem_chan_sample(None) == 0
    assert L.modem_chan_set_n0(None, 1.0) == m.ERR_INVALID_ARG and L.modem_chan_nco(None, None, None) == m.ERR_INVALID_ARG
    ch = m.Channel(n0=0.5, s0=77, device=BAD_DEVICE)                        # no device memory: no device needed
    h = ch._h
    assert L.modem_chan_process(h, None, 4, y.ctypes.data, 8, None) == m.ERR_INVALID_ARG
    assert L.modem_chan_process(h, x.ctypes.data, 4, None, 8, None) == m.ERR_INVALID_ARG      # NULL out-pointer
    assert L.modem_chan_process(h, x.ctypes.data, 8, y.ctypes.data, 7, None) == m.ERR_CAPACITY
    assert L.modem_chan_process(h, None, 0, None, 0, None) == m.MODEM_OK                      # n == 0 is a valid call
    # overlapping byte ranges that are not the in-place case
    assert L.modem_chan_process(h, x.ctypes.data, 4, x.ctypes.data + 8, 4, None) == m.ERR_INVALID_ARG
    assert L.modem_chan_process(h, x.ctypes.data + 8, 4, x.ctypes.data, 4, None) == m.ERR_INVALID_ARG
    assert ch.sample == 77                                                                  # the state is unchanged
    assert L.modem_chan_process(h, x.ctypes.data, 8, y.ctypes.data, 8, None) == m.ERR_NO_DEVICE
    assert ch.sample == 77
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(m.ModemPanic):
            ch.set_n0(bad)
    ch.set_n0(0.0)
    # in place needs equal dtypes: f32 -> f16 over the same address overlaps
    mixed = m.Channel(in_dtype=m.DTYPE_F32, out_dtype=m.DTYPE_F16, device=BAD_DEVICE)
    assert L.modem_chan_process(mixed._h, x.ctypes.data, 4, x.ctypes.data, 4, None) == m.ERR_INVALID_ARG
    # the stream must not pass sample 2^64
    top = m.Channel(s0=(1 << 64) - 2, device=BAD_DEVICE)
    assert top.sample == (1 << 64) - 2
    assert L.modem_chan_process(top._h, x.ctypes.data, 3, y.ctypes.data, 8, None) == m.ERR_INVALID_ARG
    assert top.sample == (1 << 64) - 2
    with pytest.raises(m.ModemPanic):
        m.Channel(s0=1 << 64)
    with pytest.raises(ValueError):
        ch.process(np.zeros((4, 2), np.float16))                          # not the handle's in_dtype
    with pytest.raises(ValueError):
        ch.process(x, out=np.zeros((8, 2), np.float16))


def test_count_errors_refusals(m):
    L = m.load_library()
    a = np.zeros(4, np.uint8)
    c = np.zeros(2, np.int64)
    assert L.modem_count_errors(a.ctypes.data, a.ctypes.data, 4, None, 0, None) == m.ERR_INVALID_ARG
    assert L.modem_count_errors(None, a.ctypes.data, 4, c.ctypes.data, 0, None) == m.ERR_INVALID_ARG
    assert L.modem_count_errors(a.ctypes.data, None, 4, c.ctypes.data, 0, None) == m.ERR_INVALID_ARG
    assert L.modem_count_errors(a.ctypes.data, a.ctypes.data, 4, c.ctypes.data, BAD_DEVICE, None) == m.ERR_NO_DEVICE
    with pytest.raises(m.ModemPanic):
        m.count_errors(a, np.zeros(5, np.uint8))
    with pytest.raises(ValueError):
        m.count_errors(a, a.astype(np.int8))


def _frac_turns(v):
    """frac(v / (2 pi)) of the double v, exact up to the error of PI."""
    q = Fraction(v) / (2 * PI)
    return q - math.floor(q)


@pytest.mark.parametrize("cfo", [0.0, 1e-3, -1e-3, math.pi, 2 * math.pi * 7 + 0.25, 1e6, -1e6, 1e300, 5e-324])
def test_nco_integers(m, cfo):
    ch = m.Channel(cfo=cfo, phase=-cfo, device=BAD_DEVICE)
    step, phase0 = ch.nco
    assert 0 <= step < 1 << 64 and 0 <= phase0 < 1 << 64
    for got, v in ((step, cfo), (phase0, -cfo)):
        d = (Fraction(got, 1 << 64) - _frac_turns(v)) % 1
        d = min(d, 1 - d)
        print(f"cfo {v!r}: step/2^64 off by {float(d):.3g}")
        assert d <= Fraction(1, 1 << 52)
        assert d <= Fraction(1, 1 << 64)               # what "rounded to nearest" gives: half a unit, here one
    if cfo == 0.0:
        assert step == 0 and phase0 == 0
    assert (step + phase0) % (1 << 64) == 0 or cfo == 0.0      # v and -v wrap to opposite integers


def test_identity_and_defaults(m):
    ch = m.Channel(device=BAD_DEVICE)
    assert ch.nco == (0, 0) and ch.sample == 0


# ---------------------------------------------------------------- generator statistics ----
NSTAT = 1 << 20


@pytest.fixture(scope="module")
def gauss():
    return {seed: chan_ref.noise(seed, 0, NSTAT) for seed in (0, 1, 12345)}


def test_first_word_is_prng_bits(m, o):
    """k is the first word modem_prng_bits emits for the seed (the oracle restates that generator)."""
    for seed in (0, 1, 12345, (1 << 64) - 1):
        bits = o.prng_bits(seed, 64).astype(np.uint64)
        word = int(np.sum(bits << np.arange(64, dtype=np.uint64)))
        k = int(chan_ref.mix(np.array([(seed + chan_ref.GOLDEN) & chan_ref.MASK], dtype=np.uint64))[0])
        assert k == word


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_generator_statistics(gauss, seed):
    """Each statistic within 5 standard errors of its Gaussian value (N = 2^20 complex samples)."""
    w = gauss[seed]
    N = NSTAT
    re, im = w.real, w.imag
    se = 1 / math.sqrt(N)
    stats = {
        "mean re": (re.mean(), 0.0, math.sqrt(0.5) * se),
        "mean im": (im.mean(), 0.0, math.sqrt(0.5) * se),
        "E|w|^2": ((np.abs(w) ** 2).mean(), 1.0, se),                       # |w|^2 ~ Exp(1): variance 1
        "var re": (re.var(), 0.5, 0.5 * math.sqrt(2) * se),                 # var of x^2 = 2 sigma^4
        "var im": (im.var(), 0.5, 0.5 * math.sqrt(2) * se),
        "kurt re": ((re ** 4).mean() / (re ** 2).mean() ** 2, 3.0, math.sqrt(24) * se),
        "kurt im": ((im ** 4).mean() / (im ** 2).mean() ** 2, 3.0, math.sqrt(24) * se),
        "corr re/im": ((re * im).mean() / 0.5, 0.0, se),
        "lag-1 re": ((re[1:] * re[:-1]).mean() / 0.5, 0.0, se),
        "lag-1 im": ((im[1:] * im[:-1]).mean() / 0.5, 0.0, se),
        "lag-1 re/im": ((re[1:] * im[:-1]).mean() / 0.5, 0.0, se),
    }
    for name, (got, want, s) in stats.items():
        print(f"seed {seed} {name}: {got:.6f} ({(got - want) / s:+.2f} se)")
    for name, (got, want, s) in stats.items():
        assert abs(got - want) <= 5 * s, name
    assert np.abs(w).max() <= 4.08
    assert np.abs(w).max() <= math.sqrt(24 * math.log(2)) + 1e-12


def test_seeds_are_uncorrelated(gauss):
    a, b = gauss[0], gauss[1]
    c = (a * np.conj(b)).mean()                 # E = 0, each rail's standard error sqrt(1/2N)
    print(f"cross-correlation seeds 0/1: {c:.3g}")
    assert abs(c.real) <= 5 * math.sqrt(0.5 / NSTAT) and abs(c.imag) <= 5 * math.sqrt(0.5 / NSTAT)
    assert not np.array_equal(a[:16], b[:16])


def test_generator_is_counter_based():
    a = chan_ref.noise(7, 0, 1000)
    assert np.array_equal(chan_ref.noise(7, 300, 700), a[300:])
    big = (1 << 64) - 4
    w = chan_ref.noise(7, big, 4)               # the counter wraps without complaint
    assert np.all(np.isfinite(w))


# ------------------------------------------------- the loopback band, on the CPU ----
EBN0_DB = 4.0
NBITS = 1 << 17


def loopback_band(nbits=NBITS, ebn0_db=EBN0_DB):
    ebn0 = 10.0 ** (ebn0_db / 10)
    p = 0.5 * math.erfc(math.sqrt(ebn0))
    return 1 / (2 * ebn0), nbits * p, 5 * math.sqrt(nbits * p * (1 - p))


def test_oracle_loopback_is_in_the_band(m, o):
    """QPSK, 65-tap RRC at sps 4: the oracle's TX, chan_ref.channel, the oracle's RX. The bit-error
    count must lie within 5 binomial sigmas of nbits * 0.5 erfc(sqrt(Eb/N0)) with n0 = 1/(2 Eb/N0)
    (the condition of tests/test_gpu_chan_loopback.py; the truncated filter's residual ISI is inside it)."""
    sps, L = 4, 65
    n0, want, band = loopback_band()
    taps = m.rrc_taps(L, sps, 0.35)
    w = o.sample_freq(1, 4)
    bits = o.prng_bits(0xC4A2, NBITS)
    flush = (L - 1 + sps - 1) // sps
    x = o.tx_chain(o.new_phasor(o.QPSK, 0.0, 1.0), bits, sps, taps, w, 0, flush_syms=flush)
    y, _ = chan_ref.channel(x, n0=n0, seed=2024)
    lut = o.phasor_lut(o.new_phasor(o.QPSK, 0.0, 1.0))
    _, sym = o.rx_chain(y.astype(np.float32), w, 0, o.MIX_COMPLEX, taps, sps, L - 1, o.make_slicer(o.SLICER_NEAREST, 2, lut))
    sent = bits.reshape(-1, 2) @ np.array([2, 1])
    nsym = NBITS // 2
    x_or = sym[:nsym].astype(np.int64) ^ sent
    errors = int(np.sum((x_or >> 1) + (x_or & 1)))
    print(f"oracle loopback: {errors} bit errors, expected {want:.0f} +- {band:.0f} (5 sigma)")
    assert abs(errors - want) <= band


def test_the_vectorised_rotation_equals_the_restatement():
    """chan_ref.rotate_np (numpy uint64) against chan_ref.rotate (Python integers), bit for bit."""
    rng = np.random.RandomState(5)
    for _ in range(20):
        step, phase0, s0 = (int(rng.randint(0, 1 << 32)) << 32 | int(rng.randint(0, 1 << 32)) for _ in range(3))
        assert chan_ref.rotate(step, phase0, s0, 300).tobytes() == chan_ref.rotate_np(step, phase0, s0, 300).tobytes()
    for s0 in (0, 1, (1 << 40) + 3, (1 << 64) - 2):
        assert chan_ref.rotate(3, 5, s0, 64).tobytes() == chan_ref.rotate_np(3, 5, s0, 64).tobytes()
    x = rng.randn(200, 2).astype(np.float32)
    kw = dict(gain=0.37, nco=(0x123456789ABCDEF1, 0xFEDCBA9876543210), n0=0.35, seed=99, s0=(1 << 40) + 3)
    a, b = chan_ref.channel(x, **kw), chan_ref.channel(x, rotate=chan_ref.rotate_np, **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
