"""The carrier synchronizer inside the loopback: TX -> Channel(cfo, phase, n0) -> RX -> synchronizer ->
demapper -> count_errors, the chain of tests/test_gpu_chan_loopback.py (QPSK(0, 1), sps 4, 65 taps,
2^17 bits) with a frequency offset of 1e-4 rad/sample and a phase of 0.3 rad that nothing but the
synchronizer takes out. tests/test_sync_host.py confirms the same conditions on the oracle's chain
with the restatement."""
import numpy as np
import pytest

import sync_ref

pytestmark = pytest.mark.gpu

C = sync_ref.LOOP


def _chain(m, torch, phasor, ebn0_db):
    """The received points of the whole stream, the bits sent, n0."""
    sps, L = C["sps"], C["L"]
    taps = m.rrc_taps(L, sps, 0.35)
    w = m.Freq(1, 4).sample_freq()
    n0 = sync_ref.loop_n0(phasor.lut(), ebn0_db)
    bits = m.prng_bits(C["bits_seed"], C["nbits"])
    tx = m.DigitalModulator(m.Carrier(w), phasor, sps, taps)
    ch = m.Channel(cfo=C["cfo"], phase=C["phase"], n0=n0, seed=C["noise_seed"])
    rx = m.DemodulatorRx(m.Carrier(w), taps, decim=sps, decim_offset=L - 1, mix=m.MIX_COMPLEX)
    y = torch.cat([tx.process(bits), tx.flush(like=bits)])
    ch.process(y, out=y)
    riq, _ = rx.process(y, want_sym=False)
    nsym = C["nbits"] // phasor.bits_per_symbol()
    assert riq.shape[0] >= nsym
    return riq[:nsym].contiguous(), bits, n0


def _bit_errors(m, phasor, points, bits, n0):
    llr = phasor.demapper().process(points, scale=1 / n0)
    hard = (llr < 0).to(bits.dtype).reshape(-1)
    return int(m.count_errors(hard, bits[: hard.shape[0]].contiguous()).tolist()[1])


@pytest.fixture(scope="module")
def qpsk_run(m, torch_cuda):
    qpsk = m.QPSK(0.0, 1.0)
    riq, bits, n0 = _chain(m, torch_cuda, qpsk, C["qpsk_ebn0_db"])
    assert riq.shape[0] == 65536
    out, theta, q = qpsk.synchronizer(block=C["block"]).process(riq)
    torch_cuda.cuda.synchronize()
    return dict(qpsk=qpsk, riq=riq, bits=bits, n0=n0, out=out, theta=theta, q=q)


def test_qpsk_ber_with_the_synchronizer(m, qpsk_run):
    """(a) Within 5 binomial sigmas of nbits * 0.5 erfc(sqrt(Eb/N0)) at 8 dB: a condition, not a fit."""
    r = qpsk_run
    assert r["out"].shape == (65536, 2) and r["theta"].shape == (256,)
    errors = _bit_errors(m, r["qpsk"], r["out"], r["bits"], r["n0"])
    want, band = sync_ref.ber_band(C["nbits"], C["qpsk_ebn0_db"])
    th = [int(v) & sync_ref.MASK for v in r["theta"].cpu().numpy().view(np.uint64)]
    print(f"QPSK 8 dB, cfo 1e-4, phase 0.3: {errors} bit errors in {C['nbits']}, expected {want:.0f} +- {band:.0f} (5 sigma); "
          f"min quality {float(r['q'].min()):.3f}, worst |theta - true| {sync_ref.slips(th, C['block']):.4f} turn")
    assert abs(errors - want) <= band
    assert sync_ref.slips(th, C["block"]) < 1 / 16


def test_without_the_synchronizer_the_chain_fails(m, qpsk_run):
    """(b) The same points straight into the demapper: more than 10 % bit errors."""
    r = qpsk_run
    errors = _bit_errors(m, r["qpsk"], r["riq"], r["bits"], r["n0"])
    print(f"without the synchronizer: {errors} bit errors in {C['nbits']} ({errors / C['nbits']:.1%})")
    assert errors > 0.10 * C["nbits"]


def test_qam16_has_no_slip(m, torch_cuda):
    """(c) QAM16 at 12 dB, B = 256: theta_b within 1/16 turn of the true phase at every block centre."""
    qam = m.QAM(4, 0.0, 1.0)
    riq, bits, n0 = _chain(m, torch_cuda, qam, C["qam_ebn0_db"])
    out, theta, q = qam.synchronizer(block=C["block"]).process(riq)
    th = [int(v) & sync_ref.MASK for v in theta.cpu().numpy().view(np.uint64)]
    worst = sync_ref.slips(th, C["block"])
    errors = _bit_errors(m, qam, out, bits, n0)
    print(f"QAM16 12 dB: {len(th)} blocks, min quality {float(q.min()):.3f}, worst |theta - true| {worst:.4f} turn, "
          f"{errors} bit errors in {C['nbits']}")
    assert len(th) == 128 and worst < 1 / 16
