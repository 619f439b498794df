"""The chain without knowledge of the channel: TX -> Channel(phase 0.3 + pi/2, cfo 1e-4, n0) -> RX ->
synchronizer(block 256, phase0 = 0) -> framer(guard 64, threshold 0.6) -> gather(skip 64, length 448,
power 4) -> slicer -> count_errors against the payload sent. 64 frames of a 64-symbol unique word
and 448 payload symbols, a gap of 0..99 random symbols before each (tests/frame_ref.py, LOOP).
tests/test_frame_host.py confirms the same conditions on the oracle's chain with the restatements."""
import numpy as np
import pytest

import frame_ref
import sync_ref

pytestmark = pytest.mark.gpu

C = frame_ref.LOOP


def _run(m, o, torch, phasor, ebn0_db):
    sps, L = C["sps"], C["L"]
    bps = phasor.bits_per_symbol()
    bits_np, starts, uw = frame_ref.loop_stream(o.prng_bits, bps)
    bits = torch.from_numpy(bits_np).cuda()
    taps = m.rrc_taps(L, sps, 0.35)
    w = m.Freq(1, 4).sample_freq()
    n0 = sync_ref.loop_n0(phasor.lut(), ebn0_db)
    tx = m.DigitalModulator(m.Carrier(w), phasor, sps, taps)
    ch = m.Channel(cfo=C["cfo"], phase=C["phase"], n0=n0, seed=C["noise_seed"])
    rx = m.DemodulatorRx(m.Carrier(w), taps, decim=sps, decim_offset=L - 1, mix=m.MIX_COMPLEX)
    y = torch.cat([tx.process(bits), tx.flush(like=bits)])
    ch.process(y, out=y)
    riq, _ = rx.process(y, want_sym=False)
    nsym = len(bits_np) // bps
    out, _, _ = phasor.synchronizer(block=C["block"]).process(riq[:nsym].contiguous())      # phase0 = 0
    assert out.shape[0] == nsym
    fs = phasor.framer(uw, guard=C["guard"], threshold=C["threshold"])
    assert fs.power == 4
    pos, phi, metric, count = fs.process(out, cap=128)
    sent = torch.from_numpy(frame_ref.payload_bits(bits_np, starts, bps)).cuda()
    errors = {}
    for name, ph in (("rotated", phi), ("plain", None)):
        frames, ok = fs.gather(out, 0, pos, ph, count, skip=C["uw"], length=C["payload"])
        llr = phasor.demapper().process(frames[:len(starts)].reshape(-1, 2), scale=1 / n0)
        hard = (llr < 0).to(torch.uint8).reshape(-1)
        errors[name] = int(m.count_errors(hard, sent.reshape(-1).contiguous()).tolist()[1])
        errors["ok"] = ok.cpu().numpy()
    n = int(count[0])
    ref = frame_ref.detect(out.cpu().numpy(), phasor.lut()[uw], C["guard"], C["threshold"])
    return dict(pos=pos.cpu().numpy()[:n].tolist(), metric=metric.cpu().numpy()[:n], starts=starts, errors=errors,
                nbits=int(sent.numel()), ref=ref)


def _check_hits(r, what):
    others = np.delete(r["ref"]["metric_all"], r["ref"]["pos"])
    print(f"{what}: {len(r['pos'])} hits of {len(r['starts'])} sent, min metric at a hit {r['metric'].min():.3f}, "
          f"max elsewhere {others.max():.3f}; payload bit errors {r['errors']['rotated']} of {r['nbits']}, "
          f"without the rotation {r['errors']['plain']}")
    assert r["pos"] == r["starts"] and len(r["pos"]) == 64                            # (a)
    assert r["errors"]["ok"][:64].all() and not r["errors"]["ok"][64:].any()
    assert r["metric"].min() >= 0.8 and others.max() <= 0.5                           # (b)
    assert r["ref"]["pos"] == r["starts"]


@pytest.fixture(scope="module")
def qpsk_run(m, o, torch_cuda):
    return _run(m, o, torch_cuda, m.QPSK(0.0, 1.0), C["qpsk_ebn0_db"])


def test_qpsk_frames_are_found_where_they_were_sent(qpsk_run):
    """(a), (b): exactly the 64 frame starts, metric >= 0.8 there and <= 0.5 everywhere else."""
    _check_hits(qpsk_run, "QPSK 8 dB")


def test_qpsk_payload_ber_is_the_textbook_rate(qpsk_run):
    """(c) Within 5 binomial sigmas of nbits * 0.5 erfc(sqrt(Eb/N0)) at 8 dB: a condition, not a fit."""
    want, band = sync_ref.ber_band(qpsk_run["nbits"], C["qpsk_ebn0_db"])
    print(f"{qpsk_run['errors']['rotated']} payload bit errors, expected {want:.0f} +- {band:.0f} (5 sigma)")
    assert abs(qpsk_run["errors"]["rotated"] - want) <= band


def test_without_the_rotation_the_payload_is_lost(qpsk_run):
    """(d) phi = NULL in the gather: more than 25 % bit errors, what the chain delivered before."""
    assert qpsk_run["errors"]["plain"] > 0.25 * qpsk_run["nbits"]


def test_qam16_frames_and_payload(m, o, torch_cuda):
    """(e) QAM16 at 12 dB meets (a) and (b), and its bit errors are below 1 %."""
    r = _run(m, o, torch_cuda, m.QAM(4, 0.0, 1.0), C["qam_ebn0_db"])
    _check_hits(r, "QAM16 12 dB")
    assert r["errors"]["rotated"] < 0.01 * r["nbits"]
