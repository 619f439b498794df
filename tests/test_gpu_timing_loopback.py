"""The symbol timing synchronizer inside the loopback: TX (taps sampled 1.3 samples late: a delay of
0.325 symbol) -> Channel(cfo, phase, n0) -> RX at sample rate (decim = 1) -> TimingSync(block 1024)
-> synchronizer(block 256) -> demapper -> count_errors against the bits sent, at the lag the contract
implies ((L - 1) / sps + span symbols), the first timing block skipped. QPSK(0, 1), sps 4, 65 taps,
roll-off 0.35, 2^17 bits. tests/test_timing_host.py computes the same chain on the oracle with the
restatements; its count is timing_ref.LOOP['qpsk_errors'] (profiles/timing_margins.txt)."""
import numpy as np
import pytest

import sync_ref
import timing_ref as R

pytestmark = pytest.mark.gpu

C = R.LOOP


def _received(m, torch, phasor, ebn0_db):
    """The channel's output for the whole stream, the bits sent, n0, the nominal taps."""
    sps, L = C["sps"], C["L"]
    taps = m.rrc_taps(L, sps, C["beta"])
    late = m.rrc_taps(L, sps, C["beta"], offset=C["offset"])
    w = m.Freq(1, 4).sample_freq()
    n0 = sync_ref.loop_n0(phasor.lut(), ebn0_db)
    bits = m.prng_bits(C["bits_seed"], C["nbits"])
    tx = m.DigitalModulator(m.Carrier(w), phasor, sps, late)
    ch = m.Channel(cfo=C["cfo"], phase=C["phase"], n0=n0, seed=C["noise_seed"])
    y = torch.cat([tx.process(bits), tx.flush(like=bits)])
    ch.process(y, out=y)
    return y, bits, n0, taps, w


def _bit_errors(m, phasor, points, bits, n0):
    llr = phasor.demapper().process(points.contiguous(), scale=1 / n0)
    hard = (llr < 0).to(bits.dtype).reshape(-1)
    assert hard.shape == bits.shape
    return int(m.count_errors(hard, bits.contiguous()).tolist()[1])


def test_qpsk_ber_with_and_without_the_timing_synchronizer(m, torch_cuda):
    torch = torch_cuda
    qpsk = m.QPSK(0.0, 1.0)
    y, bits, n0, taps, w = _received(m, torch, qpsk, C["qpsk_ebn0_db"])
    rx = m.DemodulatorRx(m.Carrier(w), taps, decim=1, decim_offset=0, mix=m.MIX_COMPLEX)
    riq, _ = rx.process(y, want_sym=False)
    out, tau, q = rx.timing(C["sps"], block=C["tblock"], span=C["span"]).process(riq)
    assert out.shape == (65536, 2) and tau.shape == (64,)
    pts, theta, cq = qpsk.synchronizer(block=C["block"]).process(out)
    lag, skip = R.loop_lag(), C["skip_blocks"] * C["tblock"]
    errors = _bit_errors(m, qpsk, pts[skip:], bits[2 * (skip - lag): 2 * (65536 - lag)], n0)
    want = C["qpsk_errors"]
    counted = 2 * (65536 - skip)
    band = R.binomial_band(counted, want)
    t = tau.cpu().numpy() / 2.0 ** 32
    print(f"QPSK 8 dB, taps {C['offset']} samples late: {errors} bit errors in {counted}, the oracle's chain {want} +- {band:.0f} "
          f"(5 sigma); tau mean {t.mean():.4f}, worst |tau_b - 0.325| {np.abs(t - 0.325).max():.4f}, min quality {float(q.min()):.3f}")
    assert abs(errors - want) <= band
    # without it: the RX decimates at the nominal instant
    rx2 = m.DemodulatorRx(m.Carrier(w), taps, decim=C["sps"], decim_offset=C["L"] - 1, mix=m.MIX_COMPLEX)
    riq2, _ = rx2.process(y, want_sym=False)
    pts2, _, _ = qpsk.synchronizer(block=C["block"]).process(riq2[:65536].contiguous())
    broken = _bit_errors(m, qpsk, pts2[skip:], bits[2 * skip:], n0)
    print(f"without the timing synchronizer: {broken} bit errors in {counted}")
    assert broken > 10 * errors


def test_qam16_delay_estimates(m, torch_cuda):
    """QAM16 at 12 dB: every tau_b within the recorded margin of the true 0.325 symbol."""
    torch = torch_cuda
    qam = m.QAM(4, 0.0, 1.0)
    y, bits, n0, taps, w = _received(m, torch, qam, C["qam_ebn0_db"])
    rx = m.DemodulatorRx(m.Carrier(w), taps, decim=1, decim_offset=0, mix=m.MIX_COMPLEX)
    riq, _ = rx.process(y, want_sym=False)
    out, tau, q = m.TimingSync(C["sps"], block=C["tblock"], span=C["span"]).process(riq)
    t = tau.cpu().numpy() / 2.0 ** 32
    worst = float(np.abs(t - 0.325).max())
    print(f"QAM16 12 dB: {len(t)} blocks, min quality {float(q.min()):.3f}, worst |tau_b - 0.325| {worst:.4f} symbol")
    assert len(t) == 32 and worst <= C["tau_margin"]
