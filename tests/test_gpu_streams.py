"""Stream ordering of every asynchronous entry (include/modem_hip.h, "Streams"): a call on device
buffers is queued on the stream it is given, or on torch's current stream, returns without waiting
for the device, and reads nothing back.

Every other GPU test stays on the default stream and reads its results through .cpu(), which
serialises everything; here each entry runs on side streams behind a blocker (a finite GPU-side
delay, tests/stream_util.py) with its real input arriving late:

  A  explicit stream: the input buffers hold poison, the blocker and then the copy of the real input
     are queued on S, the entry is called with stream=S while torch's current stream is the default
     one. A kernel, memset or copy that went to another stream reads the poison.
  B  the same with S made current and no stream argument.
  C  in A and B the blocker must still be running when the last call returns: the calls did not wait
     for the device. This is asserted, not assumed: it is also the premise of A and B.
  D  the current stream S1 is blocked, the entry is called with stream=S2 (idle, inputs ready) and
     only S2 is synchronised: a wrapper-side torch operation that lands on the current stream is
     caught, the second comparison after S1 drains catches a late zero-fill.
  E  two handles of one stage on two streams, their calls interleaved with different inputs.
  F  ChainBatchPlan's fork onto its own lane and the join back.

The reference of every case is the same call sequence on the default stream, on fresh handles with
identical arguments (which is also each entry's warm-up): those bytes are pinned to the float64 and
oracle references by the rest of the suite, every entry is deterministic, so all comparisons are
exact bytes. Entries that synchronise by contract (host pointers, scan_states, host-side
count_errors) are out of scope. No graph capture: the handles advance host-side counters per call.

At most two side streams (one pair for the whole file) besides the default one, and one blocker in
flight."""
import os

import numpy as np
import pytest

from conftest import product_phasor
from stream_util import Blocker, Ctx, drive, interleave, no_gc, poison

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPS, L = 4, 65                    # the c4_qpsk configuration: the matrix-core TX / RX, what the plans need
K7 = dict(K=7, polys=(0o171, 0o133), tail=True)


def _w(m):
    return m.Freq(1, 4).sample_freq()


def _iq(rng, n, dtype=np.float32):
    return rng.standard_normal((n, 2)).astype(dtype)


def _bits(rng, n):
    return rng.randint(0, 2, n).astype(np.uint8)


def _tx(m, **kw):
    return m.DigitalModulator(m.Carrier(_w(m)), product_phasor(m, "qpsk"), SPS, m.rrc_taps(L, SPS, 0.35), **kw)


def _rx(m, **kw):
    return m.DemodulatorRx(m.Carrier(_w(m)), m.rrc_taps(L, SPS, 0.35), decim=SPS, decim_offset=L - 1,
                           mix=m.MIX_COMPLEX, slicer=product_phasor(m, "qpsk").slicer(), **kw)


def _dmpsk(m):
    return m.DMPSK(2, 1.0, 0.25, float(np.float32(np.pi / 2)))


class Case:
    """One entry, or the calls of one handle. inputs(rng): the real input arrays; build(m, torch):
    fresh handles and whatever fixed buffers they own; calls(m, torch, h, x, ctx, out): a generator
    that makes one entry call per step on the device tensors x (appending the outputs to out["t"]
    and the handle state the wrapper exposes to out["state"])."""
    name = ""

    def build(self, m, torch):
        return None


class Phases(Case):
    name = "carrier_phases"            # no device input: only the bytes and the absence of a host wait are checked

    def inputs(self, rng):
        return {}

    def calls(self, m, torch, h, x, ctx, out):
        out["t"].append(m.Carrier(_w(m)).phases(12345, 5001, **ctx.kw))
        yield


class Prng(Case):
    name = "prng_bits"                 # likewise

    def inputs(self, rng):
        return {}

    def calls(self, m, torch, h, x, ctx, out):
        out["t"].append(m.prng_bits(0x5EED7000, 5001, **ctx.kw))
        yield


class Tx(Case):
    name = "tx"

    def inputs(self, rng):
        return {"b1": _bits(rng, 1001), "b2": _bits(rng, 5002)}      # an odd count: one bit carries over

    def build(self, m, torch):
        return _tx(m)

    def calls(self, m, torch, h, x, ctx, out):
        for b in (x["b1"], x["b2"]):
            out["t"].append(h.process(b, **ctx.kw))
            out["state"].append((h.carrier.sample, h._ncarry))
            yield
        out["t"].append(h.flush(like=x["b1"], **ctx.kw))
        out["state"].append(h.carrier.sample)
        yield


class TxScan(Case):
    name = "tx_dmpsk"                  # a scanned phasor: the per-symbol state buffer grows with the second call

    def inputs(self, rng):
        return {"b1": _bits(rng, 300), "b2": _bits(rng, 3001)}

    def build(self, m, torch):
        return m.DigitalModulator(m.Carrier(_w(m)), _dmpsk(m), SPS)

    def calls(self, m, torch, h, x, ctx, out):
        for b in (x["b1"], x["b2"]):
            out["t"].append(h.process(b, **ctx.kw))
            out["state"].append((h.carrier.sample, h._ncarry))
            yield


class TxBatch(Case):
    name = "tx_batch"

    def inputs(self, rng):
        return {f"b{c}": _bits(rng, 2048 + 2 * c) for c in range(3)}

    def build(self, m, torch):
        return [_tx(m) for _ in range(3)]

    def calls(self, m, torch, h, x, ctx, out):
        for _ in range(2):
            out["t"] += m.DigitalModulator.process_batch(h, [x[f"b{c}"] for c in range(3)], **ctx.kw)
            out["state"].append([t.carrier.sample for t in h])
            yield


class TxScanBatch(TxBatch):
    name = "tx_dmpsk_batch"            # the bank launch of the scanned phasors

    def build(self, m, torch):
        return [m.DigitalModulator(m.Carrier(_w(m)), _dmpsk(m), SPS) for _ in range(3)]


class TxPlan(Case):
    name = "tx_plan"

    def inputs(self, rng):
        return {f"b{c}": _bits(rng, 2048) for c in range(3)}

    def build(self, m, torch):
        mods = [_tx(m) for _ in range(3)]
        return mods, [torch.zeros((2048 // 2 * SPS, 2), dtype=torch.float32, device="cuda") for _ in mods]

    def calls(self, m, torch, h, x, ctx, out):
        mods, outs = h
        plan = out["keep"] = m.TxBatchPlan(mods, [x[f"b{c}"] for c in range(3)], outs)
        for _ in range(2):
            out["state"].append((plan.run(**ctx.kw), [t.carrier.sample for t in mods]))
            out["t"] += [ctx.snap(o) for o in outs]
            yield


class Rx(Case):
    name = "rx"

    def inputs(self, rng):
        return {"y1": _iq(rng, 1001), "y2": _iq(rng, 4099)}

    def build(self, m, torch):
        return _rx(m)

    def calls(self, m, torch, h, x, ctx, out):
        for y in (x["y1"], x["y2"]):
            out["t"] += list(h.process(y, **ctx.kw))
            out["state"].append((h.carrier.sample, h._consumed))
            yield
        out["t"] += list(h.flush(like=x["y1"], **ctx.kw))
        out["state"].append(h.carrier.sample)
        yield


class RxBatch(Case):
    name = "rx_batch"

    def inputs(self, rng):
        return {f"y{c}": _iq(rng, 4096 + 4 * c) for c in range(3)}

    def build(self, m, torch):
        return [_rx(m) for _ in range(3)]

    def calls(self, m, torch, h, x, ctx, out):
        for _ in range(2):
            for iq, sym in m.DemodulatorRx.process_batch(h, [x[f"y{c}"] for c in range(3)], **ctx.kw):
                out["t"] += [iq, sym]
            out["state"].append([r.carrier.sample for r in h])
            yield


class RxPlan(Case):
    name = "rx_plan"

    def inputs(self, rng):
        return {f"y{c}": _iq(rng, 4096) for c in range(3)}

    def build(self, m, torch):
        rxs = [_rx(m) for _ in range(3)]
        return (rxs, [torch.zeros((1024, 2), dtype=torch.float32, device="cuda") for _ in rxs],
                [torch.zeros(1024, dtype=torch.uint8, device="cuda") for _ in rxs])

    def calls(self, m, torch, h, x, ctx, out):
        rxs, oiq, osym = h
        plan = out["keep"] = m.RxBatchPlan(rxs, [x[f"y{c}"] for c in range(3)], oiq, osym)
        for _ in range(2):
            out["state"].append((plan.run(**ctx.kw), [r.carrier.sample for r in rxs]))
            out["t"] += [ctx.snap(o) for o in oiq + osym]
            yield


class Demod(Case):
    name = "demodulator"               # the reference Demodulator: the exact real mix at every sample

    def inputs(self, rng):
        return {"s1": _iq(rng, 300), "s2": _iq(rng, 3001)}

    def build(self, m, torch):
        return m.Demodulator(m.Carrier(_w(m)), m.rrc_taps(33, SPS, 0.35))

    def calls(self, m, torch, h, x, ctx, out):
        for s in (x["s1"], x["s2"]):
            out["t"].append(h.process(s, **ctx.kw))
            out["state"].append(h.carrier.sample)
            yield


class Fir(Case):
    name = "fir"

    def inputs(self, rng):
        return {"x1": rng.standard_normal(300).astype(np.float32), "x2": rng.standard_normal(3001).astype(np.float32)}

    def build(self, m, torch):
        return m.FIRFilter(m.rrc_taps(33, SPS, 0.35))

    def calls(self, m, torch, h, x, ctx, out):
        for v in (x["x1"], x["x2"]):
            out["t"].append(h.process(v, **ctx.kw))
            yield


class Demap(Case):
    name = "demap"

    def inputs(self, rng):
        return {"r": _iq(rng, 3001)}

    def build(self, m, torch):
        return m.SoftDemapper(product_phasor(m, "qam16"), out_dtype=m.DTYPE_I8)

    def calls(self, m, torch, h, x, ctx, out):
        out["t"].append(h.process(x["r"], 4.0, **ctx.kw))
        yield


class Diff(Case):
    name = "diff"

    def inputs(self, rng):
        return {"r1": _iq(rng, 300), "r2": _iq(rng, 3001)}

    def build(self, m, torch):
        return m.DiffDetector(_dmpsk(m))

    def calls(self, m, torch, h, x, ctx, out):
        for r in (x["r1"], x["r2"]):                                   # the second call starts from the first one's last point
            out["t"] += list(h.process(r, 2.0, **ctx.kw))
            yield


class Tone(Case):
    name = "tone"

    def inputs(self, rng):
        return {"x1": _iq(rng, 301), "x2": _iq(rng, 3003)}             # neither a multiple of 8: samples carry over

    def build(self, m, torch):
        return m.ToneDetector(m.MFSK(2, m.Freq(1, 16), 1.0), 8, carrier=m.Carrier(_w(m)))

    def calls(self, m, torch, h, x, ctx, out):
        for v in (x["x1"], x["x2"]):
            out["t"] += list(h.process(v, 2.0, want_energy=True, **ctx.kw))
            out["state"].append(h._ncarry)
            yield


class Chain(Case):
    name = "chain"
    NSAMP = 8200

    def inputs(self, rng):
        return {"bits": _bits(rng, self.NSAMP // SPS * 2)}

    def build(self, m, torch):
        n = self.NSAMP
        return dict(tx=_tx(m), rx=_rx(m), y=torch.zeros((n, 2), dtype=torch.float32, device="cuda"),
                    oiq=torch.zeros((n // SPS, 2), dtype=torch.float32, device="cuda"),
                    osym=torch.zeros(n // SPS, dtype=torch.uint8, device="cuda"))

    def calls(self, m, torch, h, x, ctx, out):
        plan = out["keep"] = m.ChainPlan(h["tx"], h["rx"], x["bits"], h["y"], h["oiq"], h["osym"])
        for _ in range(2):
            out["state"].append((plan.run(**ctx.kw), h["tx"].carrier.sample, h["rx"].carrier.sample))
            out["t"] += [ctx.snap(h[k]) for k in ("y", "oiq", "osym")]
            yield


class ChainBatch(Case):
    """5 channels in groups of 2: three groups, the middle one (channels 2 and 3) on the plan's own
    lane. Two runs back to back, then one copy of every channel's outputs on the caller's stream."""
    name = "chain_batch"
    NCH, GROUP, NSAMP = 5, 2, 8200

    def inputs(self, rng):
        return {f"bits{c}": _bits(rng, self.NSAMP // SPS * 2) for c in range(self.NCH)}

    def build(self, m, torch):
        n = self.NSAMP
        return [dict(tx=_tx(m), rx=_rx(m), y=torch.zeros((n, 2), dtype=torch.float32, device="cuda"),
                     oiq=torch.zeros((n // SPS, 2), dtype=torch.float32, device="cuda"),
                     osym=torch.zeros(n // SPS, dtype=torch.uint8, device="cuda")) for _ in range(self.NCH)]

    def calls(self, m, torch, h, x, ctx, out):
        plan = m.ChainBatchPlan([d["tx"] for d in h], [d["rx"] for d in h], [x[f"bits{c}"] for c in range(self.NCH)],
                                [d["y"] for d in h], [d["oiq"] for d in h], [d["osym"] for d in h], group=self.GROUP)
        out["keep"] = plan                                             # destroyed only after the comparison
        for _ in range(2):
            out["state"].append((plan.run(**ctx.kw), [d["tx"].carrier.sample for d in h]))
            yield
        fresh = [torch.empty_like(d[k]) for d in h for k in ("y", "oiq", "osym")]
        with ctx.on():
            for f, src in zip(fresh, [d[k] for d in h for k in ("y", "oiq", "osym")]):
                f.copy_(src)
        out["t"] += fresh


class Chan(Case):
    name = "channel"

    def inputs(self, rng):
        return {"x1": _iq(rng, 301), "x2": _iq(rng, 3001)}

    def build(self, m, torch):
        return m.Channel(gain=0.9, phase=0.3, cfo=0.01, n0=0.1, seed=7)

    def calls(self, m, torch, h, x, ctx, out):
        for v in (x["x1"], x["x2"]):
            out["t"].append(h.process(v, **ctx.kw))
            out["state"].append(h.sample)
            yield


class CSync(Case):
    name = "carrier_sync"              # 4 blocks of estimates, then 47: the estimate workspaces grow

    def inputs(self, rng):
        return {"r1": _iq(rng, 300), "r2": _iq(rng, 3000)}

    def build(self, m, torch):
        return m.CarrierSync(4, block=64)

    def calls(self, m, torch, h, x, ctx, out):
        for r in (x["r1"], x["r2"]):
            out["t"] += list(h.process(r, **ctx.kw))
            out["state"].append((h.symbol, h._ncarry))
            yield
        out["t"].append(h.flush(like=x["r1"], **ctx.kw))
        yield


class TSync(Case):
    name = "timing_sync"               # 2 blocks (of 32 symbols at 4 samples), then 23

    def inputs(self, rng):
        return {"x1": _iq(rng, 300), "x2": _iq(rng, 3000)}

    def build(self, m, torch):
        return m.TimingSync(4, block=32)

    def calls(self, m, torch, h, x, ctx, out):
        for v in (x["x1"], x["x2"]):
            out["t"] += list(h.process(v, **ctx.kw))
            out["state"].append((h.sample, h._ncarry))
            yield
        out["t"].append(h.flush(like=x["x1"], **ctx.kw))
        yield


class Frame(Case):
    """300 symbols (one tile of 256 positions), then 3000 (twelve): the per-tile workspaces grow while
    the first call is still queued. The hits of the second call are gathered from its buffer."""
    name = "frame_sync"
    LU, W = 16, 16

    def _uw(self):
        return np.random.RandomState(99).choice([-1.0, 1.0], (self.LU, 2)).astype(np.float32)

    def inputs(self, rng):
        x = rng.randint(-1, 2, (3300, 2)).astype(np.float32)
        for s in (40, 255, 292, 700, 1300, 1301 + 255, 2500, 3200):         # 292: across the cut between the calls
            x[s:s + self.LU] = self._uw()
        return {"x1": x[:300].copy(), "x2": x[300:].copy()}

    def build(self, m, torch):
        return m.FrameSync(self._uw(), guard=self.W, threshold=0.9)

    def _hits(self, ctx, res):
        pos, phi, met, cnt = res
        return [ctx.upto(pos, cnt), ctx.upto(phi, cnt), ctx.upto(met, cnt), cnt]

    def calls(self, m, torch, h, x, ctx, out):
        out["t"] += self._hits(ctx, h.process(x["x1"], **ctx.kw))
        out["state"].append((h.symbol, h._ncarry))
        yield
        pos, phi, met, cnt = h.process(x["x2"], **ctx.kw)
        out["t"] += self._hits(ctx, (pos, phi, met, cnt))
        out["state"].append((h.symbol, h._ncarry))
        yield
        out["t"] += list(h.gather(x["x2"], 300, pos, phi, cnt, length=32, power=4, **ctx.kw))
        yield
        out["t"] += self._hits(ctx, h.flush(like=x["x1"], **ctx.kw))
        out["state"].append((h.symbol, h._ncarry))
        yield


class Encode(Case):
    name = "conv_encode"

    def inputs(self, rng):
        return {"bits": rng.randint(0, 2, (17, 65)).astype(np.uint8)}

    def calls(self, m, torch, h, x, ctx, out):
        out["t"].append(m.ConvCode(**K7).encode(x["bits"], **ctx.kw))
        yield


class Viterbi(Case):
    name = "viterbi"                   # K = 7, 17 frames of 65 bits (one of them flagged off), then 5 more

    def inputs(self, rng):
        nc = 2 * (65 + 6)
        llr = lambda nf: np.clip(np.rint(rng.standard_normal((nf, nc)) * 40.0), -127, 127).astype(np.int8)
        ok = np.ones(17, np.uint8)
        ok[3] = 0
        return {"llr1": llr(17), "ok1": ok, "llr2": llr(5)}

    def build(self, m, torch):
        return m.ConvCode(**K7).decoder()

    def calls(self, m, torch, h, x, ctx, out):
        out["t"] += list(h.process(x["llr1"], 65, ok=x["ok1"], **ctx.kw))
        yield
        out["t"] += list(h.process(x["llr2"], 65, **ctx.kw))
        yield


class CountErrors(Case):
    name = "count_errors"              # counts=None: the wrapper zero-fills, then accumulates twice into it

    def inputs(self, rng):
        return {"a": _bits(rng, 5001), "b": _bits(rng, 5001), "c": rng.randint(0, 256, 777).astype(np.uint8),
                "d": rng.randint(0, 256, 777).astype(np.uint8)}

    def calls(self, m, torch, h, x, ctx, out):
        counts = m.count_errors(x["a"], x["b"], **ctx.kw)
        yield
        out["t"].append(m.count_errors(x["c"], x["d"], counts=counts, **ctx.kw))
        yield


CASES = [Phases(), Prng(), Tx(), TxScan(), TxBatch(), TxScanBatch(), TxPlan(), Rx(), RxBatch(), RxPlan(), Demod(),
         Fir(), Demap(), Diff(), Tone(), Chain(), ChainBatch(), Chan(), CSync(), TSync(), Frame(), Encode(), Viterbi(),
         CountErrors()]
BY_NAME = {c.name: c for c in CASES}
PAIRED = ["frame_sync", "carrier_sync", "timing_sync", "channel", "viterbi", "rx", "tx"]      # test E


def _inputs(case, seed):
    return case.inputs(np.random.RandomState(1000 + seed))


def _run(m, torch, case, x, ctx):
    """The case's calls on fresh handles; returns (handles and outputs kept alive, host seconds)."""
    h = case.build(m, torch)
    out = {"t": [], "state": [], "h": h}
    dt = drive(case.calls(m, torch, h, x, ctx, out))
    return out, dt


def _upload(torch, arrays):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()}


@pytest.fixture(scope="module")
def env(m, torch_cuda):
    """The two side streams, the calibrated blocker, every case's reference bytes and state (default
    stream, fresh handles: also each entry's first call) and the blocker length, sized from the warm
    host time of the longest call sequence."""
    torch = torch_cuda
    ref, host = {}, {}
    for case in CASES:
        for seed in ((0, 1) if case.name in PAIRED else (0,)):
            ctx = Ctx(torch)
            out, _ = _run(m, torch, case, _upload(torch, _inputs(case, seed)), ctx)
            torch.cuda.synchronize()
            ref[case.name, seed] = (ctx.read(out["t"]), out["state"])
        out, host[case.name] = _run(m, torch, case, _upload(torch, _inputs(case, 0)), Ctx(torch))   # warm: timed
        torch.cuda.synchronize()
        del out
    blocker = Blocker(torch)
    longest = max(host, key=host.get)
    ms = min(500.0, max(50.0, 20.0 * host[longest] * 1e3))
    lines = ["# tests/test_gpu_streams.py: the blocker's length against the host time of the calls it must outlast",
             f"longest warm call sequence: {longest}, {host[longest] * 1e3:.3f} ms on the host",
             f"blocker: {ms:.1f} ms (20 x that, floor 50 ms, cap 500 ms), by "
             f"{'torch.cuda._sleep' if blocker.use_sleep else 'a chain of matmuls'} at {blocker.units_per_ms:.0f} units per ms",
             f"ratio: {ms / (host[longest] * 1e3):.1f}",
             "# per case, ms on the host:"] + [f"{k}: {v * 1e3:.3f}" for k, v in host.items()]
    print("\n".join(lines))
    try:
        with open(os.path.join(ROOT, "profiles", "stream_margins.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass                                                           # a read-only checkout: the numbers were printed
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    return dict(torch=torch, ref=ref, blocker=blocker, ms=ms, s1=s1, s2=s2)


def _same(got, state, ref, what):
    rb, rs = ref
    assert state == rs, f"{what}: handle state {state} != {rs}"
    assert len(got) == len(rb), what
    for i, (g, r) in enumerate(zip(got, rb)):
        assert g == r, f"{what}: output {i} differs from the default-stream reference"


def _late(m, env, case, explicit):
    """A (explicit) or B: poison in the input buffers, then on S the blocker, the copy of the real
    input and the calls. Returns after the comparison; the premise (C) is asserted first."""
    torch, S = env["torch"], env["s1"]
    real = _inputs(case, 0)
    x = _upload(torch, {k: poison(v) for k, v in real.items()})
    src = _upload(torch, real)
    h = case.build(m, torch)
    torch.cuda.synchronize()
    out = {"t": [], "state": [], "h": h}
    ctx = Ctx(torch, S, explicit=explicit)
    with no_gc():
        ev = env["blocker"].queue(S, env["ms"])
        with torch.cuda.stream(S):
            for k in x:
                x[k].copy_(src[k])
        if explicit:
            drive(case.calls(m, torch, h, x, ctx, out))
        else:
            with torch.cuda.stream(S):
                drive(case.calls(m, torch, h, x, ctx, out))
        running = not ev.query()                                       # C: right after the last call returns
        S.synchronize()
    got = ctx.read(out["t"])
    assert running, (f"{case.name}: the blocker ({env['ms']:.0f} ms) had already ended when the calls returned: "
                     "a call waited for the device")
    _same(got, out["state"], env["ref"][case.name, 0], case.name)
    return out


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_late_input_explicit_stream(m, env, name):
    """A and C."""
    _late(m, env, BY_NAME[name], explicit=True)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_late_input_current_stream(m, env, name):
    """B and C."""
    _late(m, env, BY_NAME[name], explicit=False)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_explicit_stream_while_current_stream_is_blocked(m, env, name):
    """D: everything the entry queues must be on S2; S1, torch's current stream, is stuck behind the blocker."""
    torch, S1, S2 = env["torch"], env["s1"], env["s2"]
    case = BY_NAME[name]
    x = _upload(torch, _inputs(case, 0))
    h = case.build(m, torch)
    torch.cuda.synchronize()
    out = {"t": [], "state": [], "h": h}
    ctx = Ctx(torch, S2, explicit=True)
    with no_gc():
        ev = env["blocker"].queue(S1, env["ms"])
        with torch.cuda.stream(S1):
            drive(case.calls(m, torch, h, x, ctx, out))
        S2.synchronize()
        first = ctx.read(out["t"])
        running = not ev.query()
        S1.synchronize()
    again = ctx.read(out["t"])
    assert running, f"{name}: S2 finished only after the blocker on S1: the calls were not independent of the current stream"
    _same(first, out["state"], env["ref"][name, 0], f"{name} (S2 synchronised, S1 still blocked)")
    _same(again, out["state"], env["ref"][name, 0], f"{name} (after S1 drained)")


@pytest.mark.parametrize("name", PAIRED)
def test_two_handles_two_streams(m, env, name):
    """E: handle A on S1 (behind the blocker, so the device runs its calls after B's although the host
    issued them in turn), handle B on S2, different inputs: a workspace or state shared between
    handles would mix the two."""
    torch, S1, S2 = env["torch"], env["s1"], env["s2"]
    case = BY_NAME[name]
    xa, xb = _upload(torch, _inputs(case, 0)), _upload(torch, _inputs(case, 1))
    ha, hb = case.build(m, torch), case.build(m, torch)
    torch.cuda.synchronize()
    oa, ob = {"t": [], "state": [], "h": ha}, {"t": [], "state": [], "h": hb}
    ca, cb = Ctx(torch, S1, explicit=True), Ctx(torch, S2, explicit=True)
    with no_gc():
        env["blocker"].queue(S1, env["ms"])
        interleave(case.calls(m, torch, ha, xa, ca, oa), case.calls(m, torch, hb, xb, cb, ob))
        S2.synchronize()
        gb = cb.read(ob["t"])
        S1.synchronize()
    ga = ca.read(oa["t"])
    _same(ga, oa["state"], env["ref"][name, 0], f"{name}: handle A")
    _same(gb, ob["state"], env["ref"][name, 1], f"{name}: handle B")


def test_chain_batch_fork_and_join(m, env):
    """F: behind the blocker and the late bits, ChainBatchPlan.run(stream=S) twice back to back (every
    group stays on its lane), then one copy of every channel's outputs queued on S, and S alone
    synchronised: every channel, the side lane's included, equals the reference.

    The start event is tested deterministically: the side lane has no other reason to wait for the
    late bits, and without it the middle group would modulate the poison. The end join is exposed
    only probabilistically: without it the copies on S race the side lane's last kernels, which on
    an otherwise idle device may well have finished by then."""
    out = _late(m, env, BY_NAME["chain_batch"], explicit=True)
    case = BY_NAME["chain_batch"]
    assert len(out["t"]) == 3 * case.NCH and case.NCH > 2 * case.GROUP
