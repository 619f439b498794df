"""bench.py --dump-outputs with the real kernels: the arrays of the last timed step are the same
from run to run whatever the clock settling ran (it runs on a twin's handles), they are what the
step's caller holds (checked against the oracle's stream at that step), and an array over its
share of the byte budget is cut to the same seeded rows every time."""
import os

import numpy as np
import pytest

from conftest import ROOT, sent_symbols

pytestmark = pytest.mark.gpu

NSAMP, NCH, STEPS, WARMUP = 1 << 14, 2, 3, 1
WL = ("qam16", 4, 129, 4, NSAMP, NCH, 0, "dump: 2 channels x 2^14 C3 samples")


def _bench():
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _run(bench, outdir, settle_ms, full=False):
    bench.WORKLOADS["dump"] = WL
    args = bench.argparse.Namespace(config="dump", steps=STEPS, warmup=WARMUP, no_cpu_baseline=True, cpu_samples=0,
                                    amplitude=1.0, no_out_of_cache=True, settle_ms=settle_ms, full=full,
                                    dump_outputs=str(outdir))
    return bench.run(args, lambda wl, r: bench.GpuRunner(wl, r, 0, streams=1, batch=True))


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_the_last_step_and_repeats(torch_cuda, o, tmp_path):
    bench = _bench()
    out = _run(bench, tmp_path / "a", 0.0)
    assert out["full"] is False and out["ms_per_step"] > 0 and out["steps"] == STEPS
    assert "roofline" not in out and "decisions_match_sent" not in out and "cpu_baseline" not in out
    a = _load(tmp_path / "a")
    assert sorted(a) == [f"ch{c:02d}_{k}.npy" for c in range(NCH) for k in ("rx_iq", "rx_sym", "tx_samples")]
    # settling (a wall-time budget of steps) and the --full legs after the dump change nothing
    _run(bench, tmp_path / "b", 30.0, full=True)
    b = _load(tmp_path / "b")
    for f in a:
        assert a[f].dtype == np.float32 and np.array_equal(a[f], b[f]), f
    # the oracle's stream, STEPS + WARMUP periods of the same bits: the last period's arrays
    L, sps, bps = 129, 4, 4
    taps, w = o.rrc_taps(L, sps, 0.35), o.sample_freq(1, 4)
    nsym = NSAMP // sps
    for c in range(NCH):
        bits = o.prng_bits(bench.channel_seed(0, NCH, c), nsym * bps)
        y = o.tx_chain(o.new_phasor(o.QAM, 4, 0.0, 1.0), np.tile(bits, STEPS + WARMUP), sps, taps, w, 0)
        last = y[-NSAMP:]
        got = a[f"ch{c:02d}_tx_samples.npy"]
        assert got.shape == (NSAMP, 2)
        assert np.max(np.abs(got - last.reshape(NSAMP, 2))) <= 1e-5 * np.max(np.abs(last))
        sym = a[f"ch{c:02d}_rx_sym.npy"]
        assert sym.shape == (nsym,) and a[f"ch{c:02d}_rx_iq.npy"].shape == (nsym, 2)
        lag = (L - 1) // sps
        sent = sent_symbols(bits, bps)
        assert np.array_equal(sym.astype(np.uint8), sent[(np.arange(nsym) - lag) % nsym])


def test_outputs_sample_is_fixed_and_within_budget(torch_cuda):
    bench = _bench()
    r = bench.GpuRunner(WL, 0, 0, streams=1, batch=True)
    r.step()
    r.step()
    r.sync()
    whole = dict(r.outputs(bench.DUMP_BYTES))
    budget = 3 * NCH * 4096
    cut = r.outputs(budget)
    assert sum(a.nbytes for _, a in cut) <= budget
    again = dict(r.outputs(budget))
    idx = np.sort(np.random.default_rng(bench.SEED).choice(NSAMP, 512, replace=False))
    for name, a in cut:
        assert a.dtype == np.float32 and np.array_equal(a, again[name])
    assert np.array_equal(dict(cut)["ch01_tx_samples"], whole["ch01_tx_samples"][idx])
