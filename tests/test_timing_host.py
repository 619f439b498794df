"""Symbol timing synchronizer, host side (no device needed): the C ABI entry points exist and refuse
bad arguments before they look for a device; the offset RRC taps; the restatement of
tests/timing_ref.py alone on the generator's streams, which must recover the delay; the conditions
tests/test_gpu_timing.py puts on its inputs; and the restatements on the oracle's loopback, whose
error count tests/test_gpu_timing_loopback.py holds the device to. With TIMING_HOST_MARGINS_OUT set
the measured figures go to the file it names (they are filed in profiles/timing_margins.txt)."""
import ctypes
import math
import os

import numpy as np
import pytest

import chan_ref
import sync_ref
import timing_ref as R

BAD_DEVICE = R.BAD_DEVICE
SYMBOLS = ("modem_timing_create", "modem_timing_process", "modem_timing_flush", "modem_timing_sample",
           "modem_timing_destroy", "modem_rrc_taps_offset")
FIGURES = []


@pytest.fixture(scope="module", autouse=True)
def figures_file():
    yield
    path = os.environ.get("TIMING_HOST_MARGINS_OUT")
    if path and FIGURES:
        with open(path, "w") as f:
            f.write("# the restatement alone (tests/test_timing_host.py), float64\n")
            for line in FIGURES:
                f.write(line + "\n")


def _create(m, sps=4, block=256, span=2, tau0=0.0, flags=0, in_dtype=0, out_dtype=0, device=0, out="handle"):
    h = ctypes.c_void_p(0xDEAD)
    st = m.load_library().modem_timing_create(sps, block, span, tau0, flags, in_dtype, out_dtype, device,
                                              None if out is None else ctypes.byref(h))
    return st, h


def test_library_exports_the_timing_synchronizer(m):
    lib = ctypes.CDLL(m.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert m.load_library().modem_abi_version() == 6      # additive: the version stays
    assert "TimingSync" in m.__all__ and hasattr(m, "TimingSync") and hasattr(m.DemodulatorRx, "timing")


@pytest.mark.parametrize("device", [0, BAD_DEVICE])
def test_create_refusals_come_before_the_device(m, device):
    inf, nan = float("inf"), float("nan")
    bad = [dict(sps=0), dict(sps=1), dict(sps=2), dict(sps=3), dict(sps=6), dict(sps=16),
           dict(block=0), dict(block=16), dict(block=31), dict(block=48), dict(block=257), dict(block=8192), dict(block=1 << 31),
           dict(span=0), dict(span=17), dict(span=1 << 31),
           dict(tau0=nan), dict(tau0=inf), dict(tau0=-inf), dict(tau0=2.0000001), dict(tau0=-2.5), dict(span=1, tau0=1.5),
           dict(flags=2), dict(flags=3), dict(flags=1 << 31),
           dict(in_dtype=m.DTYPE_I16), dict(in_dtype=m.DTYPE_I8), dict(out_dtype=m.DTYPE_I16), dict(out_dtype=m.DTYPE_I8),
           dict(in_dtype=-1), dict(out_dtype=4)]
    for kw in bad:
        st, h = _create(m, device=device, **kw)
        assert st == m.ERR_INVALID_ARG, kw
        assert h.value is None, kw
    st, _ = _create(m, device=device, out=None)
    assert st == m.ERR_INVALID_ARG
    for kw in (dict(sps=5), dict(block=100), dict(span=0), dict(tau0=nan), dict(in_dtype=m.DTYPE_I8)):
        with pytest.raises(m.ModemPanic):
            m.TimingSync(**{"sps": 4, "device": device, **kw})


def test_a_bad_ordinal_is_no_device(m):
    for device in (BAD_DEVICE, -1):
        for kw in (dict(), dict(sps=8, block=32, span=16, tau0=-16.0, flags=1, in_dtype=1, out_dtype=1)):
            st, h = _create(m, device=device, **kw)
            assert st == m.ERR_NO_DEVICE and h.value is None


def test_null_handles(m):
    L = m.load_library()
    y = np.zeros((8, 2), np.float32)
    n = ctypes.c_size_t(7)
    assert L.modem_timing_process(None, y.ctypes.data, 1, y.ctypes.data, 8, None, None, 0, ctypes.byref(n), None, None) == m.ERR_INVALID_ARG
    assert n.value == 0
    assert L.modem_timing_flush(None, y.ctypes.data, 8, None, None) == m.ERR_INVALID_ARG
    assert L.modem_timing_sample(None) == 0 and L.modem_timing_destroy(None) == m.MODEM_OK


# ------------------------------------------------------------------ the offset taps ----
def _rrc64(L, sps, beta, offset):
    t = (np.arange(L) - (L - 1) / 2.0 - offset) / sps
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (np.sin(np.pi * t * (1 - beta)) + 4 * beta * t * np.cos(np.pi * t * (1 + beta))) / (np.pi * t * (1 - (4 * beta * t) ** 2))
    v = np.where(t == 0, 1 - beta + 4 * beta / np.pi, v)
    edge = np.abs(np.abs(4 * beta * t) - 1) < 1e-12
    v = np.where(edge, beta / np.sqrt(2) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * beta)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * beta))), v)
    return v / np.sqrt((v ** 2).sum())


@pytest.mark.parametrize("L,sps,beta", [(65, 4, 0.35), (129, 4, 0.25), (513, 8, 0.35), (33, 4, 0.5)])
def test_offset_taps(m, L, sps, beta):
    L_ = m.load_library()
    nominal = m.rrc_taps(L, sps, beta)
    plain = np.zeros(L, np.float32)
    assert L_.modem_rrc_taps(L, sps, beta, plain.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == m.MODEM_OK
    assert nominal.tobytes() == plain.tobytes() == m.rrc_taps(L, sps, beta, offset=0.0).tobytes()      # offset 0: bit for bit
    for offset in (0.0, 1.3, -0.7, 2.5, float(sps)):
        got = m.rrc_taps(L, sps, beta, offset=offset).astype(np.float64)
        assert abs((got ** 2).sum() - 1.0) < 1e-6                                                     # unit energy
        assert np.abs(got - _rrc64(L, sps, beta, offset)).max() <= 2.0 ** -24                          # the float64 formula, rounded to f32
    # one symbol late: the nominal taps shifted by sps, away from the edges (the energy lost at the edge rescales by < 1e-3)
    late = m.rrc_taps(L, sps, beta, offset=float(sps)).astype(np.float64)
    mid = slice(L // 4, L - L // 4)
    shifted = np.concatenate([np.zeros(sps), nominal[:-sps].astype(np.float64)])
    assert np.abs(late[mid] - shifted[mid]).max() < 2e-3 * np.abs(nominal).max()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(m.ModemPanic):
            m.rrc_taps(L, sps, beta, offset=bad)


# ------------------------------------------------- the restatement on the generator ----
def _points(kind, n, rng):
    if kind == "qpsk":
        return ((2 * rng.randint(0, 2, n) - 1) + 1j * (2 * rng.randint(0, 2, n) - 1)) / np.sqrt(2)
    lv = np.array([-3, -1, 1, 3]) / np.sqrt(10)
    return lv[rng.randint(0, 4, n)] + 1j * lv[rng.randint(0, 4, n)]


def test_reference_recovers_the_delay():
    """QPSK and 16-QAM, N = 4 and 8, tau in {-0.4, 0, 0.3}, a drift of 0.2 symbol per block; B = 256,
    roll-off 0.35, no noise: what is left is the estimator's self-noise. The worst error is measured
    and printed; the assertion is the margin chosen over it, 0.05 symbol (a tenth of the unwrap range)."""
    block, worst = 256, 0.0
    for kind in ("qpsk", "qam16"):
        for sps in (4, 8):
            for tau in (-0.4, 0.0, 0.3):
                rng = np.random.RandomState(int(1000 * (tau + 1)) + sps)
                nb = 4
                x = R.stream(_points(kind, nb * block + 2, rng), sps, nb * block * sps, tau, 0.2 / block, 0.35)
                r = R.timing(x, sps, block, 2, tau)
                kc = np.arange(nb) * block + (block - 1) / 2
                err = np.abs(np.array(r["D"]) / 2.0 ** 32 - R.true_delay(kc, tau, 0.2 / block)).max()
                worst = max(worst, float(err))
                # and the output is the symbol sequence, span symbols late (past the start-up)
                k = np.arange(block, nb * block)
                pts = _points(kind, nb * block + 2, np.random.RandomState(int(1000 * (tau + 1)) + sps))
                assert np.abs(r["out"][k] - pts[k - 2]).max() < 0.2, (kind, sps, tau)
    line = f"generator streams, B 256, roll-off 0.35, no noise: worst |tau_b - true| {worst:.4f} symbol; margin chosen 0.05"
    print(line)
    FIGURES.append(line)
    assert worst <= 0.05


def test_reference_recurrence_is_a_prefix_sum():
    rng = np.random.RandomState(3)
    Phi = [int(v) for v in rng.randint(0, 1 << 32, 50, dtype=np.uint64)]
    start = R.d_start(-1.37)
    D, _ = R.unwrap(Phi, start)
    acc, prev = start, start & 0xFFFFFFFF
    for b, p in enumerate(Phi):
        acc += R.sext32(p - prev)
        prev = p
        assert acc == D[b] and D[b] & 0xFFFFFFFF == p


@pytest.mark.parametrize("name", list(R.CASES))
def test_gpu_case_streams_keep_clear_of_the_branches(name):
    """What tests/test_gpu_timing.py asserts of its inputs, checked here on the CPU for the dtypes it uses."""
    x, sps, block = R.case_stream(name)
    for dt in (np.float32, np.float16):
        r = R.timing(R.cplx(x.astype(dt)), sps, block, R.CASE_SPAN, R.CASE_TAU0)
        assert r["q"].min() >= 0.02 and min(r["margins"]) >= 0.1
        assert max(abs(d) for d in r["D"]) < R.CASE_SPAN << 32                 # no clamp in these cases


def test_coefficients_at_zero_and_partition_of_unity():
    mu = np.linspace(0, 1, 1025)[:-1]
    c = R.coefs(mu)
    assert np.array_equal(c[0], [0, 1, 0, 0]) and np.abs(c.sum(1) - 1).max() < 1e-15
    assert np.abs(c).sum(1).max() <= 1.25                                       # what the out bound uses


# ------------------------------------------------- the loopback conditions, on the CPU ----
def _oracle_loopback(m, o, kind, ebn0_db):
    """The oracle's TX with the late taps, chan_ref.channel with the product's NCO integers, the
    oracle's RX at sample rate. Returns (riq (n, 2) float32 at sample rate, sent symbols, lut, n0)."""
    C = R.LOOP
    sps, L = C["sps"], C["L"]
    taps = m.rrc_taps(L, sps, C["beta"])
    late = m.rrc_taps(L, sps, C["beta"], offset=C["offset"])
    w = o.sample_freq(1, 4)
    bits = o.prng_bits(C["bits_seed"], C["nbits"])
    phasor = (lambda: o.new_phasor(o.QPSK, 0.0, 1.0)) if kind == "qpsk" else (lambda: o.new_phasor(o.QAM, 4, 0.0, 1.0))
    lut = o.phasor_lut(phasor())
    bps = int(lut.shape[0]).bit_length() - 1
    n0 = sync_ref.loop_n0(lut, ebn0_db)
    x = o.tx_chain(phasor(), bits, sps, late, w, 0, flush_syms=(L - 1 + sps - 1) // sps)
    nco = m.Channel(cfo=C["cfo"], phase=C["phase"], device=BAD_DEVICE).nco
    y, _ = chan_ref.channel(x, nco=nco, n0=n0, seed=C["noise_seed"])
    riq, _ = o.rx_chain(y.astype(np.float32), w, 0, o.MIX_COMPLEX, taps, 1, 0, None)
    sent = bits.reshape(-1, bps).astype(np.int64) @ (1 << np.arange(bps)[::-1])
    return riq, sent, lut, n0


def _bit_errors(points, lut, sent):
    z = points[:, 0] + 1j * points[:, 1]
    t = lut[:, 0].astype(np.float64) + 1j * lut[:, 1].astype(np.float64)
    dec = np.argmin(np.abs(z[:, None] - t[None, :]), 1)
    x = dec ^ sent
    return int(sum(((x >> j) & 1).sum() for j in range(8)))


def _synchronised(m, riq, lut):
    """Timing, then carrier, restatements. Returns (timing dict, points (nsym, 2) float64)."""
    C = R.LOOP
    t = R.timing(R.cplx(riq), C["sps"], C["tblock"], C["span"], 0.0)
    nsym = len(t["D"]) * C["tblock"]
    sym = R.pairs(t["out"][:nsym]).astype(np.float32)
    power, norm, ref = m._sync_params(lut)
    c = sync_ref.sync(sym, power, C["block"], norm, sync_ref.turns(m, ref), 0)
    return t, c["out"][:nsym]


def test_reference_qpsk_loopback_count(m, o):
    """The count tests/test_gpu_timing_loopback.py holds the device to, and the textbook count."""
    C = R.LOOP
    riq, sent, lut, _ = _oracle_loopback(m, o, "qpsk", C["qpsk_ebn0_db"])
    t, pts = _synchronised(m, riq, lut)
    lag, skip = R.loop_lag(), C["skip_blocks"] * C["tblock"]
    assert len(pts) == 65536 and lag == 18
    errors = _bit_errors(pts[skip:], lut, sent[skip - lag: len(pts) - lag])
    counted = 2 * (len(pts) - skip)
    theory = counted * 0.5 * math.erfc(math.sqrt(10.0 ** (C["qpsk_ebn0_db"] / 10)))
    tau = np.array(t["D"]) / 2.0 ** 32
    line = (f"oracle QPSK loopback 8 dB, taps {C['offset']} samples late: {errors} bit errors in {counted} (theory {theory:.0f}, "
            f"5 sigma {R.binomial_band(counted, theory):.0f}); tau mean {tau.mean():.4f} rms about 0.325 {np.sqrt(((tau - 0.325) ** 2).mean()):.4f}, "
            f"min q {t['q'].min():.3f}, min unwrap margin {min(t['margins']):.3f}")
    print(line)
    FIGURES.append(line)
    assert abs(errors - theory) <= R.binomial_band(counted, theory)
    assert abs(errors - C["qpsk_errors"]) <= math.sqrt(C["qpsk_errors"])           # the recorded count, up to libm
    # without the timing synchronizer: every 4th sample from L - 1, the nominal instant
    plain = riq[C["L"] - 1:: C["sps"]][: len(sent)].astype(np.float64)
    power, norm, ref = m._sync_params(lut)
    c = sync_ref.sync(plain.astype(np.float32), power, C["block"], norm, sync_ref.turns(m, ref), 0)
    broken = _bit_errors(c["out"][skip: 65536], lut, sent[skip: 65536])
    FIGURES.append(f"  the same chain sampled at the nominal instant (no timing synchronizer): {broken} bit errors")
    print(FIGURES[-1])
    assert broken > 10 * errors


def test_reference_qam16_loopback_delay(m, o):
    """QAM16 at 12 dB, B = 1024: every tau_b within LOOP['tau_margin'] of the true 0.325 symbol."""
    C = R.LOOP
    riq, sent, lut, _ = _oracle_loopback(m, o, "qam16", C["qam_ebn0_db"])
    t, pts = _synchronised(m, riq, lut)
    tau = np.array(t["D"]) / 2.0 ** 32
    worst = float(np.abs(tau - 0.325).max())
    line = (f"oracle QAM16 loopback 12 dB: {len(tau)} blocks of 1024, worst |tau_b - 0.325| {worst:.4f} symbol; "
            f"margin chosen {C['tau_margin']}")
    print(line)
    FIGURES.append(line)
    assert len(tau) == 32 and worst <= C["tau_margin"]


# ------------------------------------------------------- the vectorised restatement ----
@pytest.mark.parametrize("in_dtype", [0, 1])
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_the_vectorised_restatement_equals_the_restatement(name, flat, in_dtype):
    """timing_ref's *_np variants against the functions they restate, element for element, on the
    streams of tests/test_gpu_timing.py (the flush included), on the degenerate shapes, on random
    32-bit Phi (every wrap) and on delays beyond the span (the clamp)."""
    x32, sps, block = R.case_stream(name)
    z = R.cplx(x32.astype(np.float16 if in_dtype else np.float32))
    bn = block * sps
    for zs in (z, z[: bn - 1], z[:bn], z[: bn + sps + 1], z[:0]):
        a = R.timing(zs, sps, block, R.CASE_SPAN, R.CASE_TAU0, flat)
        b = R.timing_np(zs, sps, block, R.CASE_SPAN, R.CASE_TAU0, flat)
        for key in ("Phi", "D"):
            assert b[key].dtype == np.int64 and [int(v) for v in b[key]] == a[key], key
        assert np.array_equal(np.asarray(a["margins"], np.float64), b["margins"])
        for key in ("q", "turn", "out", "taps", "m", "mu24"):
            assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key
    rng = np.random.RandomState(block + sps + flat)
    Phi = [int(v) for v in rng.randint(0, 1 << 32, 300)]
    for start in (R.d_start(R.CASE_TAU0), -(5 << 32) - 12345, (7 << 32) + 99):
        D, mg = R.unwrap(Phi, start)
        D_np, mg_np = R.unwrap_np(Phi, start)
        assert [int(v) for v in D_np] == D and np.array_equal(np.asarray(mg), mg_np)
        for first in (True, False):
            pa = R.positions(D, start, sps, block, 1, flat, 7, first)
            pb = R.positions_np(D_np, start, sps, block, 1, flat, 7, first)
            assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    pa, pb = R.positions([], 12345, sps, block, 2, flat, 9), R.positions_np([], 12345, sps, block, 2, flat, 9)
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
