"""The convolutional code inside the loopback, all on the device: prng_bits -> ConvCode.encode ->
TX -> Channel -> RX -> int8 demapper -> Viterbi decoder, K = 7 (0171, 0133), 256 frames of 442
bits, QPSK at an information Eb/N0 of 3 dB. The decoder must equal the restatement on the very LLRs
it was given, the decoded errors must be at most a tenth of what uncoded QPSK makes at that Eb/N0
(tests/test_fec_host.py holds the restatement to the same condition on the oracle's chain), and the
raw errors of the coded bits must be the textbook ones at Es/N0 = R Eb/N0 per bit."""
import math

import numpy as np
import pytest

import fec_ref

pytestmark = pytest.mark.gpu

SPS, L = 4, 65
K, POLYS, NFRAMES, NBITS = 7, (0o171, 0o133), 256, 442
EBN0 = 10.0 ** 0.3                  # information bits
N0 = 1 / (2 * 0.5 * EBN0)           # QPSK of amplitude 1, 2 coded bits per symbol, rate 1/2
QS = 8.0
LIMIT = 259                         # 113152 * 0.5 erfc(sqrt(Eb/N0)) = 2589 uncoded errors expected; a tenth


def test_coded_loopback_at_3_db(m, torch_cuda):
    torch = torch_cuda
    assert round(NFRAMES * NBITS * 0.5 * math.erfc(math.sqrt(EBN0)) / 10) == LIMIT
    taps = m.rrc_taps(L, SPS, 0.35)
    w = m.Freq(1, 4).sample_freq()
    qpsk, code = m.QPSK(0.0, 1.0), m.ConvCode(K, POLYS)
    bits = m.prng_bits(0xFEC0, NFRAMES * NBITS).view(NFRAMES, NBITS)
    coded = code.encode(bits)
    ncoded = code.coded_bits(NBITS)
    assert tuple(coded.shape) == (NFRAMES, ncoded)
    tx = m.DigitalModulator(m.Carrier(w), qpsk, SPS, taps)
    y = torch.cat([tx.process(coded.view(-1)), tx.flush(like=coded)])
    m.Channel(n0=N0, seed=77).process(y, out=y)
    rx = m.DemodulatorRx(m.Carrier(w), taps, decim=SPS, decim_offset=L - 1, mix=m.MIX_COMPLEX)
    riq, _ = rx.process(y, want_sym=False)
    nsym = NFRAMES * ncoded // 2
    assert riq.shape[0] >= nsym
    llr = qpsk.demapper(out_dtype=m.DTYPE_I8).process(riq[:nsym].contiguous(), scale=QS / N0)
    got, metric = code.decoder().process(llr, NBITS, stride=ncoded)
    assert tuple(got.shape) == (NFRAMES, NBITS)
    decoded = m.count_errors(got.view(-1), bits.reshape(-1))
    raw = m.count_errors((llr.view(-1) < 0).to(torch.uint8), coded.view(-1))
    torch.cuda.synchronize()

    want_bits, want_metric = fec_ref.decode(fec_ref.quantise(llr.cpu().numpy().reshape(NFRAMES, ncoded)), NBITS, K, POLYS)
    assert np.array_equal(got.cpu().numpy(), want_bits) and np.array_equal(metric.cpu().numpy(), want_metric)

    p = 0.5 * math.erfc(math.sqrt(EBN0 / 2))                            # per coded bit: Es/N0 of a QPSK axis = R Eb/N0
    ntot = NFRAMES * ncoded
    want, band = ntot * p, 5 * math.sqrt(ntot * p * (1 - p))
    nerr, nraw = int(decoded[0]), int(raw[0])
    print(f"coded loopback at 3 dB: {nerr} decoded bit errors of {NFRAMES * NBITS} (limit {LIMIT}); "
          f"{nraw} raw errors of {ntot} coded bits, expected {want:.0f} +- {band:.0f} (5 sigma)")
    assert nerr == int(np.sum(want_bits != bits.cpu().numpy()))
    assert nerr <= LIMIT
    assert abs(nraw - want) <= band
