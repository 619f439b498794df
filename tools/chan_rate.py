#!/usr/bin/env python3
"""Cost of the channel model (Channel.process, modem_chan.hip) on 2^24 samples, by HIP events
around `--reps` back-to-back calls (median of `--windows` windows, after a warm-up), next to a
hipMemcpyAsync device-to-device copy that moves the same bytes (it reads the input's bytes and
writes as many: for equal dtypes exactly what the channel reads and writes), timed the same way in
the same process. Cases: noise only, rotation only, both; f32 -> f32 and f16 -> f16; out of place
and in place. Every call of a window works on the next of `sets` buffer sets, together larger than
`--footprint-mib` (default 600, past the 256 MiB Infinity Cache), so the rates are HBM rates.
One JSON line per case. Not run by bench.py or by any test.
Usage: tools/chan_rate.py [--n N] [--reps R] [--windows W] [--label TEXT]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # B/s, spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--footprint-mib", type=int, default=600)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    m = g.package()
    assert torch.cuda.is_available(), "chan_rate needs a GPU"
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

    kinds = [("noise", dict(n0=0.2, seed=1)), ("rot", dict(cfo=0.1234567, phase=-2.5)),
             ("both", dict(gain=0.37, cfo=0.1234567, phase=-2.5, n0=0.2, seed=1))]
    gen = torch.Generator(device="cuda").manual_seed(0xC4A2)
    for dt, tdt, name in ((m.DTYPE_F32, torch.float32, "f32"), (m.DTYPE_F16, torch.float16, "f16")):
        ssz = 2 * torch.empty(0, dtype=tdt).element_size()
        nbytes = 2 * a.n * ssz                                    # read + written
        sets = max(2, -(-a.footprint_mib * (1 << 20) // nbytes) + 1)
        xs = [torch.randn((a.n, 2), device="cuda", generator=gen).to(tdt) for _ in range(sets)]
        ys = [torch.empty((a.n, 2), dtype=tdt, device="cuda") for _ in range(sets)]

        def copy(i):
            rc = hip.hipMemcpyAsync(ys[i % sets].data_ptr(), xs[i % sets].data_ptr(), a.n * ssz, 3, stream)
            assert rc == 0, rc

        tc, _, _ = timed(copy)
        for kind, kw in kinds:
            for place in ("out of place", "in place"):
                ch = m.Channel(in_dtype=dt, out_dtype=dt, **kw)
                if place == "in place":
                    t, tmin, tmax = timed(lambda i: ch.process(xs[i % sets], out=xs[i % sets]))
                else:
                    t, tmin, tmax = timed(lambda i: ch.process(xs[i % sets], out=ys[i % sets]))
                print(json.dumps({"case": f"{kind} {name}->{name} {place}", "n": a.n, "label": a.label,
                                  "us": round(t * 1e6, 2), "us_min": round(tmin * 1e6, 2), "us_max": round(tmax * 1e6, 2),
                                  "bytes": nbytes, "tb_s": round(nbytes / t / 1e12, 3),
                                  "gsamples_s": round(a.n / t / 1e9, 1),
                                  "frac_of_8tb_s": round(nbytes / t / HBM_PEAK, 3),
                                  "copy_same_bytes_us": round(tc * 1e6, 2), "vs_copy": round(t / tc, 2),
                                  "buffer_sets": sets}), flush=True)
        del xs, ys


if __name__ == "__main__":
    main()
