"""Rate matching and the frame check inside the loopback, all on the device.

Rate 3/4: prng_bits -> CRC.ccitt16().attach -> ConvCode(7).encode -> RateMatch.tx (3/4, 32 columns)
-> QPSK TX -> Channel -> RX -> int8 demapper (QS = 8) -> RateMatch.rx -> Viterbi decoder ->
CRC.check, 256 frames of 442 information bits at an information Eb/N0 of 4.5 dB. The decoder must
equal the restatement on the very LLRs the device produced, ok' the restatement's check of the
decoded rows, the decoded errors must be at most a tenth of what uncoded QPSK makes at that Eb/N0,
a frame that passes the CRC must be free of errors, and the raw errors of the transmitted bits must
be the textbook ones (tests/test_ratematch_host.py holds the restatement to the same conditions on
the oracle's chain, with the same seeds).

Burst: 64 noiseless frames whose transmitted LLRs 200 .. 223 are erased: with 32 columns every
frame decodes and passes, with one column the device still equals the restatement and frames fail."""
import math

import numpy as np
import pytest

import fec_ref
import ratematch_ref as R

pytestmark = pytest.mark.gpu

SPS, L = 4, 65
K, POLYS, NFRAMES, NBITS, W = 7, (0o171, 0o133), 256, 442, 16
NM = 2 * (NBITS + W + K - 1)        # 928 mother bits of a frame
E = 619                             # of them transmitted at rate 3/4
RATE = NBITS / E                    # information bits over transmitted coded bits: the CRC and the tail are overhead
EBN0 = 10.0 ** 0.45                 # information bits
N0 = 1 / (2 * RATE * EBN0)          # QPSK of amplitude 1, 2 coded bits per symbol: n0 = 1 / (2 R Eb/N0)
QS = 8.0
LIMIT = 100                         # 113152 * 0.5 erfc(sqrt(Eb/N0)) = 995 uncoded errors expected; a tenth


def test_rate_3_4_coded_loopback_at_4_5_db(m, torch_cuda):
    torch = torch_cuda
    assert round(NFRAMES * NBITS * 0.5 * math.erfc(math.sqrt(EBN0)) / 10) == LIMIT
    taps = m.rrc_taps(L, SPS, 0.35)
    w = m.Freq(1, 4).sample_freq()
    qpsk, code, crc = m.QPSK(0.0, 1.0), m.ConvCode(K, POLYS), m.CRC.ccitt16()
    rm = code.rate_match(m.PUNCTURE_3_4, cols=32)
    bits = m.prng_bits(0xC0DE, NFRAMES * NBITS).view(NFRAMES, NBITS)
    coded = code.encode(crc.attach(bits))
    assert tuple(coded.shape) == (NFRAMES, NM) and rm.kept(NM) == E == R.kept(R.PUNCTURE_3_4, NM)
    sent = rm.tx(coded)
    assert tuple(sent.shape) == (NFRAMES, E)
    tx = m.DigitalModulator(m.Carrier(w), qpsk, SPS, taps)
    y = torch.cat([tx.process(sent.view(-1)), tx.flush(like=sent)])
    m.Channel(n0=N0, seed=78).process(y, out=y)
    rx = m.DemodulatorRx(m.Carrier(w), taps, decim=SPS, decim_offset=L - 1, mix=m.MIX_COMPLEX)
    riq, _ = rx.process(y, want_sym=False)
    nsym = NFRAMES * E // 2
    assert riq.shape[0] >= nsym
    llr = qpsk.demapper(out_dtype=m.DTYPE_I8).process(riq[:nsym].contiguous(), scale=QS / N0).view(NFRAMES, E)
    mother = rm.rx(llr, NM)
    got, metric = code.decoder().process(mother, NBITS + W)
    ok = crc.check(got)
    decoded = m.count_errors(got[:, :NBITS].contiguous().view(-1), bits.reshape(-1))
    raw = m.count_errors((llr.reshape(-1) < 0).to(torch.uint8), sent.view(-1))
    torch.cuda.synchronize()

    bits_np, llr_np, got_np = bits.cpu().numpy(), llr.cpu().numpy(), got.cpu().numpy()
    want_mother = R.rx(llr_np, NM, R.PUNCTURE_3_4, 32)
    assert np.array_equal(mother.cpu().numpy(), want_mother)
    want_bits, want_metric = fec_ref.decode(fec_ref.quantise(want_mother), NBITS + W, K, POLYS)
    assert np.array_equal(got_np, want_bits) and np.array_equal(metric.cpu().numpy(), want_metric)
    ok_np = ok.cpu().numpy()
    assert np.array_equal(ok_np, R.check(got_np, 16, 0x1021, 0xFFFF))

    p = 0.5 * math.erfc(math.sqrt(RATE * EBN0))                         # per transmitted bit: Es/N0 of a QPSK axis = R Eb/N0
    ntot = NFRAMES * E
    want, band = ntot * p, 5 * math.sqrt(ntot * p * (1 - p))
    nerr, nraw = int(decoded[0]), int(raw[0])
    wrong = (got_np[:, :NBITS] != bits_np).sum(1)
    print(f"rate-3/4 loopback at 4.5 dB: {nerr} decoded bit errors of {NFRAMES * NBITS} (limit {LIMIT}) in {int((wrong > 0).sum())} "
          f"frames, {int(ok_np.sum())} frames pass the CRC; {nraw} raw errors of {ntot} transmitted bits, expected "
          f"{want:.0f} +- {band:.0f} (5 sigma)")
    assert nerr == int(wrong.sum())
    assert nerr <= LIMIT
    assert not wrong[ok_np == 1].any()
    assert abs(nraw - want) <= band


@pytest.mark.parametrize("pattern", [(1,), R.PUNCTURE_3_4])
def test_a_burst_of_erasures_needs_the_interleaver(m, torch_cuda, pattern):
    torch = torch_cuda
    nframes = 64
    code, crc = m.ConvCode(K, POLYS), m.CRC.ccitt16()
    bits = m.prng_bits(0xB0B5, nframes * NBITS).view(nframes, NBITS)
    framed = crc.attach(bits)
    coded = code.encode(framed)
    dec = code.decoder()
    passed = {}
    for cols in (32, 1):
        rm = code.rate_match(pattern, cols=cols)
        llr = (64 - 128 * rm.tx(coded).to(torch.int16)).to(torch.int8)  # +-64
        llr[:, 200:224] = 0
        mother = rm.rx(llr, NM)
        got, metric = dec.process(mother, NBITS + W)
        ok = crc.check(got)
        want_mother = R.rx(llr.cpu().numpy(), NM, pattern, cols)
        assert np.array_equal(mother.cpu().numpy(), want_mother)
        want_bits, want_metric = fec_ref.decode(fec_ref.quantise(want_mother), NBITS + W, K, POLYS)
        assert np.array_equal(got.cpu().numpy(), want_bits) and np.array_equal(metric.cpu().numpy(), want_metric)
        assert np.array_equal(ok.cpu().numpy(), R.check(want_bits, 16, 0x1021, 0xFFFF))
        if cols == 32:
            assert torch.equal(got, framed)
        passed[cols] = int(ok.sum())
    print(f"burst of 24 erasures, pattern of {len(pattern)}: frames of {nframes} that pass the CRC: {passed}")
    assert passed[32] == nframes and passed[1] < nframes
