"""Carrier synchronizer, host side (no device needed): the C ABI entry points exist and refuse bad
arguments before they look for a device; the M / norm / ref_phase that `.synchronizer()` derives
from a table; sync_atan2_turn against double (tools/sync_math_check.cpp, compiled here); and the
restatement of tests/sync_ref.py alone on the oracle's loopback, which must meet the conditions
tests/test_gpu_sync_loopback.py puts on the device."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import chan_ref
import sync_ref
from conftest import ROOT

BAD_DEVICE = 1 << 20
SYMBOLS = ("modem_sync_create", "modem_sync_process", "modem_sync_flush", "modem_sync_symbol", "modem_sync_destroy")


def _create(m, power=4, block=256, norm=1.0, ref_phase=0.0, phase0=0.0, flags=0, in_dtype=0, out_dtype=0, device=0,
            out="handle"):
    h = ctypes.c_void_p(0xDEAD)
    st = m.load_library().modem_sync_create(power, block, norm, ref_phase, phase0, flags, in_dtype, out_dtype, device,
                                            None if out is None else ctypes.byref(h))
    return st, h


def test_library_exports_the_synchronizer(m):
    lib = ctypes.CDLL(m.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert m.load_library().modem_abi_version() == 6      # additive: the version stays
    assert "CarrierSync" in m.__all__ and hasattr(m, "CarrierSync")
    assert hasattr(m.QPSK(0.0, 1.0), "synchronizer")


@pytest.mark.parametrize("device", [0, BAD_DEVICE])
def test_create_refusals_come_before_the_device(m, device):
    inf, nan = float("inf"), float("nan")
    bad = [dict(power=0), dict(power=1), dict(power=3), dict(power=6), dict(power=16),
           dict(block=0), dict(block=32), dict(block=63), dict(block=96), dict(block=257), dict(block=8192), dict(block=1 << 31),
           dict(norm=0.0), dict(norm=-1.0), dict(norm=nan), dict(norm=inf), dict(norm=-inf),
           dict(ref_phase=nan), dict(ref_phase=inf), dict(phase0=nan), dict(phase0=-inf),
           dict(flags=2), dict(flags=1 << 31),
           dict(in_dtype=m.DTYPE_I16), dict(in_dtype=m.DTYPE_I8), dict(out_dtype=m.DTYPE_I16), dict(out_dtype=m.DTYPE_I8),
           dict(in_dtype=-1), dict(out_dtype=4)]
    for kw in bad:
        st, h = _create(m, device=device, **kw)
        assert st == m.ERR_INVALID_ARG, kw
        assert h.value is None, kw
    st, _ = _create(m, device=device, out=None)
    assert st == m.ERR_INVALID_ARG
    for kw in (dict(power=3), dict(block=100), dict(norm=0.0), dict(phase0=nan), dict(in_dtype=m.DTYPE_I8)):
        with pytest.raises(m.ModemPanic):
            m.CarrierSync(**{"power": 4, "device": device, **kw})


def test_a_bad_ordinal_is_no_device(m):
    """The handle owns device memory, so a valid description on a device that does not exist is
    NO_DEVICE (every argument refusal above came first)."""
    for device in (BAD_DEVICE, -1):
        st, h = _create(m, device=device)
        assert st == m.ERR_NO_DEVICE and h.value is None


def test_null_handles(m):
    L = m.load_library()
    y = np.zeros((8, 2), np.float32)
    n = ctypes.c_size_t(7)
    assert L.modem_sync_process(None, y.ctypes.data, 1, y.ctypes.data, 8, None, None, 0, ctypes.byref(n), None, None) == m.ERR_INVALID_ARG
    assert n.value == 0
    assert L.modem_sync_flush(None, y.ctypes.data, 8, None, None) == m.ERR_INVALID_ARG
    assert L.modem_sync_symbol(None) == 0 and L.modem_sync_destroy(None) == m.MODEM_OK


PHASORS = {
    "bpsk": (lambda m: m.BPSK(0.7853982, 1.0), 2, None),
    "qpsk": (lambda m: m.QPSK(0.0, 1.0), 4, None),
    "qam16": (lambda m: m.QAM(4, 0.0, 1.0), 4, math.pi),
    "qam64": (lambda m: m.QAM(6, 0.0, 1.0), 4, math.pi),
    "qam256": (lambda m: m.QAM(8, 0.0, 1.0), 4, math.pi),
    "8psk": (lambda m: m.MPSK(3, 0.0, 1.0), 8, None),
}


@pytest.mark.parametrize("name", list(PHASORS))
def test_power_and_reference_of_the_constellations(m, name):
    make, power, ref = PHASORS[name]
    ph = make(m)
    lut = ph.lut().astype(np.float64)
    got_power, norm, got_ref = m._sync_params(ph.lut())
    z = lut[:, 0] + 1j * lut[:, 1]
    assert got_power == power
    assert norm == pytest.approx(1 / math.sqrt(np.mean(np.abs(z) ** 2)), rel=1e-12)
    line = ((norm * z) ** power).sum()
    strength = abs(line) / np.abs((norm * z) ** power).sum()
    print(f"{name}: M {got_power}, line strength {strength:.3f}, ref {got_ref:.6f}")
    assert strength >= 0.25
    for lower in (p for p in (2, 4) if p < power):                 # and no smaller power qualifies
        assert abs(((norm * z) ** lower).sum()) / np.abs((norm * z) ** lower).sum() < 0.25
    assert got_ref == pytest.approx(math.atan2(line.imag, line.real), abs=1e-12)
    if ref is not None:
        assert abs(abs(got_ref) - ref) < 1e-6                      # pi for square QAM (either sign of the f32 dust)


def test_a_table_without_a_line_is_refused(m):
    ring = np.exp(2j * np.pi * np.arange(16) / 16)                 # 16-PSK: no line at M <= 8
    with pytest.raises(m.ModemPanic):
        m._sync_params(np.stack([ring.real, ring.imag], 1))
    with pytest.raises(m.ModemPanic):
        m._sync_params(np.zeros((4, 2)))
    with pytest.raises(m.ModemError):
        m.DMPSK(2, 1.0, 0.0, 1.5707964).synchronizer()


def test_atan2_turn_against_double(tmp_path):
    """tools/sync_math_check.cpp: 2^24 random pairs with magnitudes 2^-120 .. 2^120, the axes, the
    octant boundaries and their neighbours, zeros and non-finite input; the bound is 2^-22 turn."""
    exe = str(tmp_path / "sync_math_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                    "-I", os.path.join(ROOT, "rust-modem_amd", "csrc"), os.path.join(ROOT, "tools", "sync_math_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    worst = float(r.stdout.split("worst error")[1].split()[0])
    assert 0 < worst <= 2.0 ** -22


def test_reference_recurrence_is_a_prefix_sum():
    """theta_b - phase0 is the sum of the local terms, whatever the grouping: the restatement's
    serial loop against a cumulative sum of the terms mod 2^64."""
    rng = np.random.RandomState(3)
    Phi = [int(v) << 32 for v in rng.randint(0, 1 << 32, 50, dtype=np.uint64)]
    for power in (2, 4, 8):
        phase0 = 0x123456789ABCDEF0
        theta, _ = sync_ref.unwrap(Phi, power, phase0)
        lm = power.bit_length() - 1
        prev, acc = (power * phase0) & sync_ref.MASK, phase0
        for b, p in enumerate(Phi):
            acc = (acc + (sync_ref.sext(p - prev) >> lm)) & sync_ref.MASK
            prev = p
            assert acc == theta[b]
            assert abs(sync_ref.sext(power * theta[b] - p)) < power * (b + 2)     # M theta_b is Phi_b up to the dropped bits


# ------------------------------------------------- the loopback conditions, on the CPU ----
def _oracle_loopback(m, o, kind, ebn0_db):
    """The oracle's TX, chan_ref.channel with the product's NCO integers, the oracle's RX.
    Returns (riq (nsym, 2) float32, sent symbols, lut, n0)."""
    C = sync_ref.LOOP
    sps, L = C["sps"], C["L"]
    taps = m.rrc_taps(L, sps, 0.35)
    w = o.sample_freq(1, 4)
    bits = o.prng_bits(C["bits_seed"], C["nbits"])
    phasor = (lambda: o.new_phasor(o.QPSK, 0.0, 1.0)) if kind == "qpsk" else (lambda: o.new_phasor(o.QAM, 4, 0.0, 1.0))
    lut = o.phasor_lut(phasor())
    bps = int(lut.shape[0]).bit_length() - 1
    n0 = sync_ref.loop_n0(lut, ebn0_db)
    x = o.tx_chain(phasor(), bits, sps, taps, w, 0, flush_syms=(L - 1 + sps - 1) // sps)
    nco = m.Channel(cfo=C["cfo"], phase=C["phase"], device=BAD_DEVICE).nco
    y, _ = chan_ref.channel(x, nco=nco, n0=n0, seed=C["noise_seed"])
    riq, _ = o.rx_chain(y.astype(np.float32), w, 0, o.MIX_COMPLEX, taps, sps, L - 1, None)
    nsym = C["nbits"] // bps
    sent = bits.reshape(-1, bps).astype(np.int64) @ (1 << np.arange(bps)[::-1])
    return riq[:nsym], sent, lut, n0


def _bit_errors(points, lut, sent):
    """Nearest table point in float64, then the bits that differ."""
    z = points[:, 0] + 1j * points[:, 1]
    t = lut[:, 0].astype(np.float64) + 1j * lut[:, 1].astype(np.float64)
    dec = np.argmin(np.abs(z[:, None] - t[None, :]), 1)
    x = dec ^ sent
    return int(sum(((x >> j) & 1).sum() for j in range(8)))


def test_reference_meets_the_qpsk_loopback_conditions(m, o):
    """(a) and (b) of tests/test_gpu_sync_loopback.py on the oracle's chain with the restatement: the
    bit errors inside the 5-sigma band of the textbook rate, more than 10 % without the synchronizer,
    q_b >= 0.3, unwrap margins >= 0.1 turn, no slip."""
    C = sync_ref.LOOP
    riq, sent, lut, _ = _oracle_loopback(m, o, "qpsk", C["qpsk_ebn0_db"])
    power, norm, ref = m._sync_params(lut)
    assert power == 4
    r = sync_ref.sync(riq, power, C["block"], norm, sync_ref.turns(m, ref), 0)
    assert len(r["theta"]) == len(riq) // C["block"] == 256
    errors = _bit_errors(r["out"], lut, sent)
    plain = _bit_errors(riq.astype(np.float64), lut, sent)
    want, band = sync_ref.ber_band(C["nbits"], C["qpsk_ebn0_db"])
    worst = sync_ref.slips(r["theta"], C["block"])
    kc = np.arange(len(r["theta"])) * C["block"] + (C["block"] - 1) / 2
    resid = np.array([t / 2.0 ** 64 for t in r["theta"]]) - sync_ref.loop_true_phase(kc)
    resid = (resid - np.round(resid)) * 2 * np.pi
    print(f"reference QPSK loopback: {errors} bit errors, expected {want:.0f} +- {band:.0f} (5 sigma); without the "
          f"synchronizer {plain} ({plain / C['nbits']:.1%}); min q {r['q'].min():.3f}, min unwrap margin "
          f"{min(r['margins']):.3f} turn, residual phase sigma {resid.std():.4f} rad, worst |theta - true| {worst:.4f} turn")
    assert abs(errors - want) <= band
    assert plain > 0.10 * C["nbits"]
    assert r["q"].min() >= 0.3 and min(r["margins"]) >= 0.1
    assert worst < 1 / 16


def test_reference_meets_the_qam16_loopback_conditions(m, o):
    """(c): QAM16 at 12 dB, B = 256: theta_b within 1/16 turn of the true phase at every block centre."""
    C = sync_ref.LOOP
    riq, sent, lut, _ = _oracle_loopback(m, o, "qam16", C["qam_ebn0_db"])
    power, norm, ref = m._sync_params(lut)
    r = sync_ref.sync(riq, power, C["block"], norm, sync_ref.turns(m, ref), 0)
    worst = sync_ref.slips(r["theta"], C["block"])
    print(f"reference QAM16 loopback: {len(r['theta'])} blocks, min q {r['q'].min():.3f}, min unwrap margin "
          f"{min(r['margins']):.3f} turn, worst |theta - true| {worst:.4f} turn; "
          f"{_bit_errors(r['out'], lut, sent)} bit errors")
    assert len(r["theta"]) == 128
    assert worst < 1 / 16


# ------------------------------------------------------- the vectorised restatement ----
@pytest.mark.parametrize("in_dtype", [0, 1])
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("name", ["bpsk", "qpsk", "qam16", "8psk"])
def test_the_vectorised_restatement_equals_the_restatement(m, name, flat, in_dtype):
    """sync_ref's *_np variants against the functions they restate, element for element, on the
    streams of tests/test_gpu_sync.py (the flush included), on a stream with a wrap in every
    block, and on the degenerate shapes."""
    import test_gpu_sync as G
    x32, power, block = G.stream(m, name)
    x = x32.astype(G.NP_DT[in_dtype])
    sy = dict(bpsk=m.BPSK(0.7853982, 1.0), qpsk=m.QPSK(0.0, 1.0), qam16=m.QAM(4, 0.0, 1.0), **{"8psk": m.MPSK(3, 0.0, 1.0)})[name]
    _, norm, ref_phase = m._sync_params(sy.lut())
    ref, phase0 = sync_ref.turns(m, ref_phase), sync_ref.turns(m, G.PHASE0)
    for xs in (x, x[: block - 1], x[:block], x[:0]):
        a = sync_ref.sync(xs, power, block, norm, ref, phase0, flat)
        b = sync_ref.sync_np(xs, power, block, norm, ref, phase0, flat)
        assert b["Phi"].dtype == np.uint64 and b["theta"].dtype == np.uint64 and b["ph"].dtype == np.uint64
        for key in ("Phi", "theta", "ph"):
            assert [int(v) for v in b[key]] == a[key], key
        assert np.array_equal(np.asarray(a["margins"], np.float64), b["margins"])
        for key in ("q", "turn", "out"):
            assert a[key].tobytes() == b[key].tobytes(), key
        assert [int(v) for v in sync_ref.top32_np(b["ph"])] == sync_ref.top32(a["ph"])
    # arbitrary 64-bit Phi: every wrap, both signs, the shifts of negative differences
    rng = np.random.RandomState(power + flat)
    Phi = [int(v) for v in rng.randint(0, 1 << 32, 300).astype(np.uint64) << np.uint64(32) | rng.randint(0, 1 << 32, 300).astype(np.uint64)]
    th, mg = sync_ref.unwrap(Phi, power, phase0)
    th_np, mg_np = sync_ref.unwrap_np(np.array(Phi, np.uint64), power, phase0)
    assert [int(v) for v in th_np] == th and np.array_equal(np.asarray(mg), mg_np)
    assert [int(v) for v in sync_ref.phases_np(th_np, block, phase0, flat, 5)] == sync_ref.phases(th, block, phase0, flat, 5)
