#!/usr/bin/env python3
"""Cost of the symbol timing synchronizer (TimingSync.process, modem_timing.hip) on 2^20 symbols, by
HIP events around `--reps` back-to-back calls (median of `--windows` windows, after a warm-up), next
to a hipMemcpyAsync device-to-device copy of the same bytes (nsym * N samples in + nsym symbols out)
timed the same way in the same process. Cases: f32 and f16, N = 4 / 8, B = 32 / 256 / 4096. Every
call of a window works on the next of `sets` buffer sets, together larger than `--footprint-mib`
(default 600, past the 256 MiB Infinity Cache), so the rates are HBM rates. One JSON line per case.
The kernels' shares come from a kernel trace of this tool (`--trace-case` runs one case only, a few
calls, for that). Not run by bench.py or by any test.
Usage: tools/timing_rate.py [--n NSYM] [--reps R] [--windows W] [--label TEXT] [--trace-case NAME]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--footprint-mib", type=int, default=600)
    ap.add_argument("--label", default="")
    ap.add_argument("--trace-case", default="")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    m = g.package()
    assert torch.cuda.is_available(), "timing_rate needs a GPU"
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

    gen = torch.Generator(device="cuda").manual_seed(0x71)
    for dt, tdt, name in ((m.DTYPE_F32, torch.float32, "f32"), (m.DTYPE_F16, torch.float16, "f16")):
        ssz = 2 * torch.empty(0, dtype=tdt).element_size()
        for sps in (4, 8):
            nsamp = a.n * sps
            nbytes = (nsamp + a.n) * ssz                       # read once + written (the estimator reads again)
            sets = max(2, -(-a.footprint_mib * (1 << 20) // nbytes) + 1)
            # Gaussian scatter: the cost does not depend on the values
            xs = [torch.randn((nsamp, 2), device="cuda", generator=gen).to(tdt) for _ in range(sets)]
            ys = [torch.empty((a.n, 2), dtype=tdt, device="cuda") for _ in range(sets)]
            cin = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            couts = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(sets)]

            def copy(i):
                rc = hip.hipMemcpyAsync(couts[i % sets].data_ptr(), cin.data_ptr(), nbytes // 2, 3, stream)
                assert rc == 0, rc

            tc, _, _ = timed(copy)                              # nbytes / 2 read + nbytes / 2 written
            for block in (32, 256, 4096):
                case = f"N{sps} B{block} {name}->{name}"
                if a.trace_case and a.trace_case != case:
                    continue
                ts = m.TimingSync(sps, block=block, in_dtype=dt, out_dtype=dt)
                if a.trace_case:
                    for i in range(4):
                        ts.process(xs[i % sets], out=ys[i % sets])
                    torch.cuda.synchronize()
                    continue
                t, tmin, tmax = timed(lambda i: ts.process(xs[i % sets], out=ys[i % sets]))
                print(json.dumps({"case": case, "nsym": a.n, "label": a.label,
                                  "us": round(t * 1e6, 2), "us_min": round(tmin * 1e6, 2), "us_max": round(tmax * 1e6, 2),
                                  "bytes": nbytes, "tb_s": round(nbytes / t / 1e12, 3),
                                  "gsymbols_s": round(a.n / t / 1e9, 3),
                                  "copy_same_bytes_us": round(tc * 1e6, 2), "vs_copy": round(t / tc, 2),
                                  "buffer_sets": sets}), flush=True)
            del xs, ys, couts, cin


if __name__ == "__main__":
    main()
