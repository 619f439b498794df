#!/usr/bin/env python3
"""Cost of the Viterbi decoder (ViterbiDecoder.process, modem_fec.hip) and of the encoder, by HIP
events around `--reps` back-to-back calls (median of `--windows` windows, after a warm-up). Cases:
K = 7 rate 1/2 (0171, 0133) with 442-bit frames at 64, 1024 and 16384 frames, and K = 3 (7, 5) and
K = 9 (0753, 0561) at 1024 frames; int8 LLRs, uniform random (the cost does not depend on the
values), the tail on. Beside them the host decoder of tests/cpp/fec_host.cpp (the same
modem_fec_math.h, g++ -O2, one core) on 256 frames of each code, as the CPU baseline. One JSON line
per case: frames/s and information Mbit/s. Not run by bench.py or by any test.
Usage: tools/fec_rate.py [--reps R] [--windows W] [--label TEXT] [--no-cpu]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NBITS = 442
CASES = ((7, (0o171, 0o133), 64), (7, (0o171, 0o133), 1024), (7, (0o171, 0o133), 16384), (3, (7, 5), 1024),
         (9, (0o753, 0o561), 1024))


def cpu_rate(K, polys, nframes=256):
    """frames/s of the host decoder on one core."""
    with tempfile.TemporaryDirectory() as d:
        exe, fin, fout = (os.path.join(d, n) for n in ("fec_host", "in.bin", "out.bin"))
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "rust-modem_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "fec_host.cpp"), "-o", exe], check=True)
        stride = len(polys) * (NBITS + K - 1)
        np.random.RandomState(K).randint(-128, 128, (nframes, stride)).astype(np.int8).tofile(fin)
        best = None
        for _ in range(3):
            out = subprocess.run([exe, str(K), "1", str(NBITS), str(nframes), str(stride), fin, fout, *[str(g) for g in polys]],
                                 check=True, capture_output=True, text=True).stdout
            sec = float(re.search(r"in ([0-9.]+) s", out).group(1))
            best = sec if best is None else min(best, sec)
        return nframes / best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--label", default="")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    m = g.package()
    assert torch.cuda.is_available(), "fec_rate needs a GPU"

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

    gen = torch.Generator(device="cuda").manual_seed(0xFEC)
    cpu = {}
    for K, polys, nframes in CASES:
        code = m.ConvCode(K, polys)
        dec = code.decoder()
        ncoded = code.coded_bits(NBITS)
        llr = torch.randint(-128, 128, (nframes, ncoded), device="cuda", generator=gen, dtype=torch.int16).to(torch.int8)
        bits = torch.randint(0, 2, (nframes, NBITS), device="cuda", generator=gen, dtype=torch.int16).to(torch.uint8)
        t, tmin, tmax = timed(lambda: dec.process(llr, NBITS))
        te, _, _ = timed(lambda: code.encode(bits))
        if not a.no_cpu and (K, polys) not in cpu:
            cpu[K, polys] = cpu_rate(K, polys)
        c = cpu.get((K, polys))
        print(json.dumps({"case": f"K{K} r1/{len(polys)} {NBITS}-bit x{nframes}", "label": a.label,
                          "decode_us": round(t * 1e6, 2), "us_min": round(tmin * 1e6, 2), "us_max": round(tmax * 1e6, 2),
                          "frames_s": round(nframes / t, 1), "info_mbit_s": round(nframes * NBITS / t / 1e6, 2),
                          "trellis_steps_s": round(nframes * code.steps(NBITS) / t, 1),
                          "encode_us": round(te * 1e6, 2),
                          "cpu_one_core_frames_s": None if c is None else round(c, 1),
                          "cpu_one_core_info_mbit_s": None if c is None else round(c * NBITS / 1e6, 3),
                          "vs_cpu_one_core": None if c is None else round(nframes / t / c, 1)}), flush=True)


if __name__ == "__main__":
    main()
