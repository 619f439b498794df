#!/usr/bin/env python3
"""Cost of the frame synchronizer (FrameSync.process, modem_frame.hip) on 2^22 symbols, by HIP
events around `--reps` back-to-back calls (median of `--windows` windows, after a warm-up), next to
a hipMemcpyAsync device-to-device copy of the same nsym * (8 or 4) input bytes timed the same way in
the same process, and next to the f32 vector-ALU bound of 8 L flop per symbol at 157.3 TFLOP/s.
Cases: L = 16 / 64 / 256 with W = L, f32 and f16. Every call of a window works on the next of `sets`
input buffers, together larger than `--footprint-mib` (default 600, past the 256 MiB Infinity
Cache), so the bytes come from HBM. One JSON line per case. The kernels' shares come from a kernel
trace of this tool (`--trace-case` runs one case only, a few calls, for that; a run of its own, no
counters). Not run by bench.py or by any test.
Usage: tools/frame_rate.py [--n N] [--reps R] [--windows W] [--label TEXT] [--trace-case NAME]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PEAK = 157.3e12   # f32 flop/s, spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--footprint-mib", type=int, default=600)
    ap.add_argument("--label", default="")
    ap.add_argument("--trace-case", default="")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    m = g.package()
    assert torch.cuda.is_available(), "frame_rate needs a GPU"
    hip = ctypes.CDLL("libamdhip64.so")        # the runtime torch already loaded
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for i in range(3):
            fn(i)
        ts = []
        for _ in range(a.windows):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(a.reps):
                fn(i)
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1e-3 / a.reps)
        return sorted(ts)[len(ts) // 2], min(ts), max(ts)

    gen = torch.Generator(device="cuda").manual_seed(0xF5)
    qpsk = m.QPSK(0.0, 1.0)
    for dt, tdt, name in ((m.DTYPE_F32, torch.float32, "f32"), (m.DTYPE_F16, torch.float16, "f16")):
        ssz = 2 * torch.empty(0, dtype=tdt).element_size()
        nbytes = a.n * ssz
        sets = max(2, -(-a.footprint_mib * (1 << 20) // nbytes) + 1)
        # Gaussian scatter: a handful of candidates at most, the cost does not depend on the values
        xs = [torch.randn((a.n, 2), device="cuda", generator=gen).to(tdt) for _ in range(sets)]
        couts = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(2)]

        def copy(i):
            rc = hip.hipMemcpyAsync(couts[i % 2].data_ptr(), xs[i % sets].data_ptr(), nbytes, 3, stream)
            assert rc == 0, rc

        tc, _, _ = timed(copy)
        for L in (16, 64, 256):
            case = f"L{L} W{L} {name}"
            if a.trace_case and a.trace_case != case:
                continue
            fs = qpsk.framer(np.random.RandomState(L).randint(0, 4, L), in_dtype=dt)
            if a.trace_case:
                for i in range(4):
                    fs.process(xs[i % sets], cap=1024)
                torch.cuda.synchronize()
                continue
            t, tmin, tmax = timed(lambda i: fs.process(xs[i % sets], cap=1024))
            bound = 8.0 * L * a.n / VALU_PEAK
            print(json.dumps({"case": case, "n": a.n, "label": a.label,
                              "us": round(t * 1e6, 2), "us_min": round(tmin * 1e6, 2), "us_max": round(tmax * 1e6, 2),
                              "gsymbols_s": round(a.n / t / 1e9, 2), "tflops_8L": round(8.0 * L * a.n / t / 1e12, 2),
                              "valu_bound_us": round(bound * 1e6, 2), "vs_valu_bound": round(t / bound, 2),
                              "copy_same_bytes_us": round(tc * 1e6, 2), "vs_copy": round(t / tc, 2),
                              "buffer_sets": sets}), flush=True)
        del xs, couts


if __name__ == "__main__":
    main()
