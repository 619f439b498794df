"""Stream ordering of the four asynchronous entries of rate matching and the frame check
(CRC.attach, RateMatch.tx, RateMatch.rx, CRC.check), with the plumbing of tests/stream_util.py.

A file of its own, named to be collected after tests/test_gpu_streams.py: that file's test D needs
its pair of side streams and the streams of the handles under test to find hardware queues of their
own, and the runtime hands a process's streams out over a few queues in the order of their first
use. A side stream used earlier in the process would take one of them."""
import numpy as np
import pytest

import ratematch_ref as R
from stream_util import Blocker, no_gc, poison

pytestmark = pytest.mark.gpu


def test_entries_are_ordered_on_their_stream(m, torch_cuda):
    """The four entries on a side stream behind a producer: the input buffers hold poison until a copy
    queued on that stream, behind a finite GPU-side delay, brings the real input; the calls follow
    with no synchronisation in between, must return while the delay still runs, and must see the
    real input."""
    torch = torch_cuda
    rng = np.random.RandomState(9)
    rm, crc = m.RateMatch(R.PUNCTURE_3_4, cols=32), m.CRC.ccitt16()
    real = {"bits": rng.randint(0, 2, (33, 458)).astype(np.uint8), "coded": rng.randint(0, 2, (33, 928)).astype(np.uint8),
            "llr": rng.randint(-128, 128, (33, 619)).astype(np.int8)}
    real["framed"] = R.attach(rng.randint(0, 2, (33, 458)).astype(np.uint8), 16, 0x1021, 0xFFFF)
    real["framed"][::4, 17] ^= 1
    real["ok"] = (np.arange(33) % 3 != 0).astype(np.uint8)
    want = [R.attach(real["bits"], 16, 0x1021, 0xFFFF), R.tx(real["coded"], R.PUNCTURE_3_4, 32),
            R.rx(real["llr"], 928, R.PUNCTURE_3_4, 32), R.check(real["framed"], 16, 0x1021, 0xFFFF, ok=real["ok"])]
    src = {k: torch.from_numpy(v).cuda() for k, v in real.items()}
    x = {k: torch.from_numpy(poison(v)).cuda() for k, v in real.items()}
    S = torch.cuda.Stream()
    blocker = Blocker(torch)
    outs = [torch.zeros(w.shape, dtype=getattr(torch, w.dtype.name), device="cuda") for w in want]
    torch.cuda.synchronize()
    with no_gc():
        ev = blocker.queue(S, 100.0)
        with torch.cuda.stream(S):
            for k in x:
                x[k].copy_(src[k])
        crc.attach(x["bits"], out=outs[0], stream=S)
        rm.tx(x["coded"], out=outs[1], stream=S)
        rm.rx(x["llr"], 928, out=outs[2], stream=S)
        crc.check(x["framed"], ok=x["ok"], out=outs[3], stream=S)
        running = not ev.query()
        S.synchronize()
    assert running, "the delay had already ended when the calls returned: a call waited for the device"
    for i, (o, w) in enumerate(zip(outs, want)):
        assert np.array_equal(o.cpu().numpy(), w), f"entry {i} did not see the input its stream produced"
