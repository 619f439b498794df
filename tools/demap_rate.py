#!/usr/bin/env python3
"""Cost of the soft demapper (SoftDemapper.process, modem_demap.hip) at C3's symbol count
(2^22), by HIP events around `--reps` back-to-back calls (median of `--windows` windows, after a
warm-up), next to a hipMemcpyAsync device-to-device copy that moves the same bytes (a copy of
half the demapper's read + written bytes: it reads them once and writes them once), timed the
same way in the same process. Algorithmic bytes = nsym * (8 or 4) in + nsym * bps * sizeof(out).
Every call of a window works on the next of `sets` buffer sets, together larger than
`--footprint-mib` (default 600, past the 256 MiB Infinity Cache), so the rates are HBM rates.
One JSON line per case. Not run by bench.py or by any test.
Usage: tools/demap_rate.py [--nsym N] [--reps R] [--windows W] [--label TEXT]"""
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
    ap.add_argument("--nsym", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--footprint-mib", type=int, default=600)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    m = g.package()
    assert torch.cuda.is_available(), "demap_rate needs a GPU"
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

    rings = [m.Ring(range(0, 4), 0.5, 0.7853982), m.Ring(range(4, 16), 1.0, 0.2617994)]
    cases = [
        ("qam16 f32->f32", lambda: m.QAM(4, 0.0, 1.0), m.DTYPE_F32, m.DEMAP_AUTO),
        ("qam16 f32->f16", lambda: m.QAM(4, 0.0, 1.0), m.DTYPE_F16, m.DEMAP_AUTO),
        ("qam16 f32->i8", lambda: m.QAM(4, 0.0, 1.0), m.DTYPE_I8, m.DEMAP_AUTO),
        ("qam256 f32->f32", lambda: m.QAM(8, 0.0, 1.0), m.DTYPE_F32, m.DEMAP_AUTO),
        ("qam256 f32->f32 forced general", lambda: m.QAM(8, 0.0, 1.0), m.DTYPE_F32, m.DEMAP_GENERAL),
        ("apsk16 f32->f32", lambda: m.APSK(1.0, 4, rings), m.DTYPE_F32, m.DEMAP_AUTO),
    ]
    tdt = {m.DTYPE_F32: torch.float32, m.DTYPE_F16: torch.float16, m.DTYPE_I8: torch.int8}
    gen = torch.Generator(device="cuda").manual_seed(0xD3A9)
    for name, mk, odt, path in cases:
        ph = mk()
        dm = ph.demapper(out_dtype=odt, path=path)
        lut = torch.from_numpy(ph.lut()).cuda()
        esz = torch.empty(0, dtype=tdt[odt]).element_size()
        nbytes = a.nsym * 8 + a.nsym * dm.bps * esz
        sets = max(2, -(-a.footprint_mib * (1 << 20) // nbytes) + 1)
        sigma = 0.3 * float(np.min(np.linalg.norm(ph.lut()[1:] - ph.lut()[0], axis=1)))
        iqs, outs = [], []
        for _ in range(sets):
            s = torch.randint(0, lut.shape[0], (a.nsym,), device="cuda", generator=gen)
            iqs.append(lut[s] + sigma * torch.randn((a.nsym, 2), device="cuda", generator=gen))
            outs.append(torch.empty((a.nsym, dm.bps), dtype=tdt[odt], device="cuda"))
        t, tmin, tmax = timed(lambda i: dm.process(iqs[i % sets], 4.0, out=outs[i % sets]))
        half = nbytes // 2
        src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(sets)]
        dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(sets)]

        def copy(i):
            rc = hip.hipMemcpyAsync(dst[i % sets].data_ptr(), src[i % sets].data_ptr(), half, 3, stream)
            assert rc == 0, rc

        tc, _, _ = timed(copy)
        print(json.dumps({"case": name, "path": dm.path, "nsym": a.nsym, "bps": dm.bps, "label": a.label,
                          "us": round(t * 1e6, 2), "us_min": round(tmin * 1e6, 2), "us_max": round(tmax * 1e6, 2),
                          "bytes": nbytes, "tb_s": round(nbytes / t / 1e12, 3),
                          "frac_of_8tb_s": round(nbytes / t / HBM_PEAK, 3),
                          "copy_same_bytes_us": round(tc * 1e6, 2), "vs_copy": round(t / tc, 2),
                          "buffer_sets": sets}), flush=True)
        del iqs, outs, src, dst


if __name__ == "__main__":
    main()
