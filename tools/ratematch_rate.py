#!/usr/bin/env python3
"""Cost of the two new RX stages next to the Viterbi decoder they surround (RateMatch.rx and
CRC.check, modem_ratematch.hip; ViterbiDecoder.process, modem_fec.hip), by HIP events around
`--reps` back-to-back calls (median of `--windows` windows, after a warm-up). The case: 4096 frames
of 442 + 16 bits, K = 7 (0171, 0133) with the tail (928 mother bits), rate 3/4 (619 transmitted),
32 columns, int8 LLRs, uniform random (no cost depends on the values). Measured: rm_rx alone with
the bytes it moves per second (E read + Nm written per frame), crc.check alone, the decoder alone
(its code is the yardstick: this stage did not change it), and rm_rx + decoder + crc.check back to
back. Beside them the TX side: crc.attach and rm_tx. One JSON line. Not run by bench.py or by any
test. Usage: tools/ratematch_rate.py [--reps R] [--windows W] [--frames N] [--label TEXT]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NBITS, W, COLS = 442, 16, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    m = g.package()
    assert torch.cuda.is_available(), "ratematch_rate needs a GPU"

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(a.windows):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(a.reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1e-3 / a.reps)
        return sorted(ts)[len(ts) // 2], min(ts), max(ts)

    nframes = a.frames
    gen = torch.Generator(device="cuda").manual_seed(0x3A7E)
    code, crc = m.ConvCode(), m.CRC.ccitt16()
    rm = code.rate_match(m.PUNCTURE_3_4, cols=COLS)
    dec = code.decoder()
    nm = code.coded_bits(NBITS + W)
    e = rm.kept(nm)
    llr = torch.randint(-128, 128, (nframes, e), device="cuda", generator=gen, dtype=torch.int16).to(torch.int8)
    bits = torch.randint(0, 2, (nframes, NBITS), device="cuda", generator=gen, dtype=torch.int16).to(torch.uint8)
    framed = crc.attach(bits)
    coded = code.encode(framed)
    mother = torch.empty((nframes, nm), dtype=torch.int8, device="cuda")
    sent = torch.empty((nframes, e), dtype=torch.uint8, device="cuda")
    ok = torch.empty((nframes,), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(framed)
    rm.rx(llr, nm, out=mother)
    got, _ = dec.process(mother, NBITS + W)

    def chain():
        rm.rx(llr, nm, out=mother)
        d, _ = dec.process(mother, NBITS + W)
        crc.check(d, out=ok)

    t_rx = timed(lambda: rm.rx(llr, nm, out=mother))
    t_chk = timed(lambda: crc.check(got, out=ok))
    t_dec = timed(lambda: dec.process(mother, NBITS + W))
    t_all = timed(chain)
    t_att = timed(lambda: crc.attach(bits, out=out))
    t_tx = timed(lambda: rm.tx(coded, out=sent))
    us = lambda t: [round(v * 1e6, 2) for v in t]                        # noqa: E731
    print(json.dumps({"case": f"K7 r3/4 cols{COLS} {NBITS}+{W}-bit x{nframes} int8 (Nm {nm}, E {e})", "label": a.label,
                      "reps": a.reps, "windows": a.windows, "us": "median, min, max",
                      "rm_rx_us": us(t_rx), "rm_rx_gbyte_s": round(nframes * (e + nm) / t_rx[0] / 1e9, 2),
                      "crc_check_us": us(t_chk), "viterbi_us": us(t_dec), "rm_rx_viterbi_crc_check_us": us(t_all),
                      "new_stages_share_of_viterbi": round((t_rx[0] + t_chk[0]) / t_dec[0], 4),
                      "chain_over_viterbi": round(t_all[0] / t_dec[0], 4),
                      "crc_attach_us": us(t_att), "rm_tx_us": us(t_tx)}), flush=True)


if __name__ == "__main__":
    main()
