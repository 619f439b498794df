#!/usr/bin/env python3
"""Cost of the noncoherent detectors (DiffDetector.process and ToneDetector.process,
modem_noncoh.hip), by HIP events around `--reps` back-to-back calls (median of `--windows`
windows, after a warm-up), next to a hipMemcpyAsync device-to-device copy that moves the same
bytes (a copy of half the detector's read + written bytes: it reads them once and writes them
once), timed the same way in the same process.
  diff  2^22 symbols, bps 1, 2, 4:  bytes = nsym * (8 in + 1 sym + bps * 4 llr)
  fsk   (bps, sps) = (1, 8), (4, 16), (8, 256), about 2^25 samples each:
        bytes = nsym * (sps * 8 in + 1 sym + bps * 4 llr); no energy output.
        Also complex MACs per second (nsym * sps * 2^bps per call, 4 FMAs = 8 FLOP each) against
        the 157.3 TFLOP/s f32 vector peak.
Every call of a window works on the next of `sets` buffer sets, together larger than
`--footprint-mib` (default 600, past the 256 MiB Infinity Cache), so the rates are HBM rates.
One JSON line per case. Not run by bench.py or by any test.
Usage: tools/noncoh_rate.py [--reps R] [--windows W] [--label TEXT]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # B/s, spec
F32_VALU_PEAK = 157.3e12  # FLOP/s, spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsym", type=int, default=1 << 22, help="symbols per call of the differential cases")
    ap.add_argument("--nsamp", type=int, default=1 << 25, help="samples per call of the tone-bank cases")
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--footprint-mib", type=int, default=600)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    m = g.package()
    assert torch.cuda.is_available(), "noncoh_rate needs a GPU"
    hip = ctypes.CDLL("libamdhip64.so")        # the runtime torch already loaded
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn, reps):
        for i in range(3):
            fn(i)
        ts = []
        for _ in range(a.windows):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(reps):
                fn(i)
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1e-3 / reps)
        return sorted(ts)[len(ts) // 2], min(ts), max(ts)

    def copy_time(nbytes, sets, reps):
        half = nbytes // 2
        src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(sets)]
        dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(sets)]

        def copy(i):
            rc = hip.hipMemcpyAsync(dst[i % sets].data_ptr(), src[i % sets].data_ptr(), half, 3, stream)
            assert rc == 0, rc

        return timed(copy, reps)[0]

    def report(name, t, tmin, tmax, nbytes, tc, sets, **extra):
        row = {"case": name, "label": a.label, "us": round(t * 1e6, 2), "us_min": round(tmin * 1e6, 2),
               "us_max": round(tmax * 1e6, 2), "bytes": nbytes, "tb_s": round(nbytes / t / 1e12, 3),
               "frac_of_8tb_s": round(nbytes / t / HBM_PEAK, 3), "copy_same_bytes_us": round(tc * 1e6, 2),
               "vs_copy": round(t / tc, 2), "buffer_sets": sets}
        row.update(extra)
        print(json.dumps(row), flush=True)

    gen = torch.Generator(device="cuda").manual_seed(0xD1FF)
    for bps in (1, 2, 4):
        ph = m.DMPSK(bps, 1.0, 0.7853982, float(np.float32(2 * np.pi / (1 << bps))))
        det = ph.detector()
        n = a.nsym
        nbytes = n * (8 + 1 + 4 * bps)
        sets = max(2, -(-a.footprint_mib * (1 << 20) // nbytes) + 1)
        iqs, syms, llrs = [], [], []
        for _ in range(sets):
            s = torch.randint(0, 1 << bps, (n,), device="cuda", generator=gen)
            phi = torch.cumsum(s.to(torch.float64) * ph._shift, 0) + 0.7853982
            iq = torch.stack([torch.cos(phi), torch.sin(phi)], 1).to(torch.float32)
            iqs.append(iq + 0.15 * torch.randn((n, 2), device="cuda", generator=gen))
            syms.append(torch.empty(n, dtype=torch.uint8, device="cuda"))
            llrs.append(torch.empty((n, bps), dtype=torch.float32, device="cuda"))
        t, tmin, tmax = timed(lambda i: det.process(iqs[i % sets], 4.0, out_sym=syms[i % sets], out_llr=llrs[i % sets]),
                              a.reps)
        tc = copy_time(nbytes, sets, a.reps)
        report(f"diff bps {bps} f32->u8+f32", t, tmin, tmax, nbytes, tc, sets, nsym=n, bps=bps,
               msym_s=round(n / t / 1e6, 1))
        del iqs, syms, llrs

    for bps, sps, mk in ((1, 8, lambda: m.BFSK(m.Freq(1, 8), 1.0)),
                         (4, 16, lambda: m.MFSK(4, m.Freq(1, 32), 1.0, "default")),
                         (8, 256, lambda: m.MFSK(8, m.Freq(1, 512), 1.0, "increase"))):
        ph = mk()
        det = ph.detector(sps, 0.3)
        n = a.nsamp // sps
        nbytes = n * (sps * 8 + 1 + 4 * bps)
        sets = max(2, -(-a.footprint_mib * (1 << 20) // nbytes) + 1)
        reps = a.reps if bps < 8 else max(2, a.reps // 6)     # the bps 8 call is compute-bound: fewer per window
        om = torch.from_numpy(det.omega.astype(np.float64)).cuda()
        xs, syms, llrs = [], [], []
        for _ in range(sets):
            s = torch.randint(0, 1 << bps, (n,), device="cuda", generator=gen)
            arg = om[s][:, None] * torch.arange(sps, device="cuda", dtype=torch.float64)[None, :]
            x = torch.stack([torch.cos(arg), torch.sin(arg)], 2).to(torch.float32).reshape(n * sps, 2)
            xs.append(x + 0.5 * torch.randn((n * sps, 2), device="cuda", generator=gen))
            syms.append(torch.empty(n, dtype=torch.uint8, device="cuda"))
            llrs.append(torch.empty((n, bps), dtype=torch.float32, device="cuda"))
            del arg, x
        t, tmin, tmax = timed(lambda i: det.process(xs[i % sets], 1.0, out_sym=syms[i % sets], out_llr=llrs[i % sets]),
                              reps)
        tc = copy_time(nbytes, sets, a.reps)
        macs = n * sps * (1 << bps)
        report(f"fsk bps {bps} sps {sps} f32->u8+f32", t, tmin, tmax, nbytes, tc, sets, nsym=n, bps=bps, sps=sps,
               msamp_s=round(n * sps / t / 1e6, 1), gcmac_s=round(macs / t / 1e9, 1),
               frac_of_f32_valu_peak=round(8 * macs / t / F32_VALU_PEAK, 3))
        del xs, syms, llrs


if __name__ == "__main__":
    main()
