"""The channel model inside the loopback: TX -> Channel -> RX with a known N0. The bit-error rate
of QPSK at a given Eb/N0 must be the textbook one, the demapper's LLRs with scale = 1/n0 must be
calibrated against the errors actually made, and a frequency offset must be undone by its negative
and tolerated by the differential detector."""
import math

import numpy as np
import pytest

import chan_ref

pytestmark = pytest.mark.gpu

SPS, L = 4, 65
NBITS = 1 << 17
EBN0 = 10.0 ** (4.0 / 10)
N0 = 1 / (2 * EBN0)            # QPSK of amplitude 1, unit-energy matched taps: Eb = 1/2


@pytest.fixture(scope="module")
def awgn_run(m, o, torch_cuda):
    """One run shared by the BER and the calibration test: the received points, the decisions,
    the symbols sent and the error counts (counted on the device)."""
    torch = torch_cuda
    taps = m.rrc_taps(L, SPS, 0.35)
    w = m.Freq(1, 4).sample_freq()
    qpsk = m.QPSK(0.0, 1.0)
    bits = m.prng_bits(0xC4A2, NBITS)
    tx = m.DigitalModulator(m.Carrier(w), qpsk, SPS, taps)
    ch = m.Channel(n0=N0, seed=2024)
    rx = m.DemodulatorRx(m.Carrier(w), taps, decim=SPS, decim_offset=L - 1, mix=m.MIX_COMPLEX, slicer=qpsk.slicer())
    y = torch.cat([tx.process(bits), tx.flush(like=bits)])
    ch.process(y, out=y)
    riq, rsym = rx.process(y)
    nsym = NBITS // 2
    assert rsym.shape[0] >= nsym and ch.sample == y.shape[0]
    b = bits.view(-1, 2)
    sent = (b[:, 0] * 2 + b[:, 1]).to(torch.uint8)
    counts = m.count_errors(rsym[:nsym].contiguous(), sent)       # a symbol's XOR holds its bit errors
    torch.cuda.synchronize()
    return dict(riq=riq[:nsym].contiguous(), rsym=rsym[:nsym].cpu().numpy(), sent=sent.cpu().numpy(),
                counts=counts.tolist(), qpsk=qpsk)


def test_qpsk_ber_at_4_db(awgn_run):
    """Within 5 binomial sigmas of nbits * 0.5 erfc(sqrt(Eb/N0)): a condition, not a fit. (The
    oracle's TX and RX around chan_ref.channel sit in the same band: tests/test_chan_host.py.)"""
    p = 0.5 * math.erfc(math.sqrt(EBN0))
    want, band = NBITS * p, 5 * math.sqrt(NBITS * p * (1 - p))
    nsymerr, nbiterr = awgn_run["counts"]
    x = awgn_run["rsym"].astype(np.int64) ^ awgn_run["sent"]
    print(f"QPSK 4 dB: {nbiterr} bit errors in {NBITS}, expected {want:.0f} +- {band:.0f} (5 sigma); {nsymerr} symbols")
    assert nbiterr == int(np.sum((x >> 1) + (x & 1))) and nsymerr == int(np.count_nonzero(x))
    assert abs(nbiterr - want) <= band


def test_llrs_are_calibrated(m, awgn_run):
    """scale = 1/n0 makes the max-log LLRs (exact for QPSK) log-likelihood ratios: the predicted
    error probabilities 1 / (1 + e^|llr|) must add up to the errors made. A factor 2 in the noise
    variance fails this and the BER test."""
    riq = awgn_run["riq"]
    llr = awgn_run["qpsk"].demapper().process(riq, scale=1 / N0).cpu().numpy().astype(np.float64)
    r = riq.cpu().numpy().astype(np.float64)
    hard = (llr < 0).astype(np.int64)
    dec = np.stack([awgn_run["rsym"] >> 1, awgn_run["rsym"] & 1], 1).astype(np.int64)
    # f32 bound of an LLR: the two squared distances each carry a few 2^-24 of their size
    tol = (1 / N0) * 2.0 ** -20 * ((np.abs(r[:, 0]) + 1) ** 2 + (np.abs(r[:, 1]) + 1) ** 2)
    sure = np.abs(llr) > tol[:, None]
    assert np.array_equal(hard[sure], dec[sure]) and sure.mean() > 0.999
    p = 1 / (1 + np.exp(np.abs(llr)))
    sent = np.stack([awgn_run["sent"] >> 1, awgn_run["sent"] & 1], 1).astype(np.int64)
    errors = int(np.sum(hard != sent))
    want, band = p.sum(), 5 * math.sqrt(np.sum(p * (1 - p)))
    print(f"calibration: {errors} errors, sum of predicted probabilities {want:.1f} +- {band:.1f} (5 sigma)")
    assert abs(errors - want) <= band
    half = 1 / (1 + np.exp(np.abs(llr) / 2))                       # what n0 twice too small would claim
    assert abs(errors - half.sum()) > 5 * math.sqrt(np.sum(half * (1 - half)))


def test_cfo_is_undone_by_its_negative(m, torch_cuda):
    torch = torch_cuda
    taps = m.rrc_taps(L, SPS, 0.35)
    tx = m.DigitalModulator(m.Carrier(m.Freq(1, 4).sample_freq()), m.QPSK(0.0, 1.0), SPS, taps)
    x = tx.process(m.prng_bits(5, 1 << 13))
    c = 0.0123
    there, back = m.Channel(cfo=c, phase=0.4, s0=1 << 33), m.Channel(cfo=-c, phase=-0.4, s0=1 << 33)
    s1, p1 = there.nco
    s2, p2 = back.nco
    assert (s1 + s2) % (1 << 64) == 0 and (p1 + p2) % (1 << 64) == 0
    y = back.process(there.process(x))
    xs, ys = x.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)
    mod = np.hypot(xs[:, 0], xs[:, 1])
    ratio = (np.abs(ys - xs) / (2 * (2.0 ** -20 * mod + 1e-30))[:, None]).max()
    print(f"cfo there and back: worst error / (2 x parity bound) = {ratio:.3f}")
    assert ratio <= 1.0


def test_diff_detector_tolerates_a_small_cfo(m, torch_cuda):
    """DMPSK through a channel with cfo = 1e-4 rad/sample and no noise: every bit is recovered."""
    torch = torch_cuda
    sps, bps = 4, 2
    ph = m.DMPSK(bps, 1.0, 0.7853982, 1.5707964)
    fr = m.Freq(1000, 10000)
    bits = m.prng_bits(77, 4096 * bps)
    tx = m.DigitalModulator(m.Carrier(fr), ph, sps, None)
    y = m.Channel(cfo=1e-4).process(tx.process(bits))
    rx = m.DemodulatorRx(m.Carrier(fr), np.ones(4, np.float32) / 4, decim=sps, decim_offset=sps - 1, mix=m.MIX_COMPLEX)
    riq, _ = rx.process(y, want_sym=False)
    sym, _ = ph.detector().process(riq)
    b = bits.view(-1, bps)
    sent = (b[:, 0] * 2 + b[:, 1]).to(torch.uint8)
    assert sym.shape[0] == sent.shape[0]
    assert m.count_errors(sym, sent).tolist() == [0, 0]
