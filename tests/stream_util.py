"""Plumbing of tests/test_gpu_streams.py: a finite GPU-side delay (the blocker), poison values, and the
context that says on which stream a case's calls and its own torch operations go.

Nothing here waits for the host to release the device: the blocker is `torch.cuda._sleep` (a spin
kernel that ends after a cycle count) or, where this torch lacks it, a fixed chain of matmuls. Its
length per unit is measured once with events, so a blocker of a wanted duration can be queued."""
import contextlib
import gc
import time

import numpy as np


class Blocker:
    """queue(stream, ms) puts a delay of about `ms` milliseconds on `stream` and returns an event
    recorded right behind it: event.query() is False while the delay is still running."""

    def __init__(self, torch):
        self.torch = torch
        self.use_sleep = hasattr(torch.cuda, "_sleep")
        if not self.use_sleep:
            self.a = torch.randn(1024, 1024, device="cuda") * (1.0 / 32.0)
        self._unit(1)                                    # code object, lazy allocations
        torch.cuda.synchronize()
        probe = 20_000_000 if self.use_sleep else 50     # cycles / matmuls
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        self._unit(probe)
        t1.record()
        t1.synchronize()
        self.units_per_ms = probe / max(t0.elapsed_time(t1), 1e-3)

    def _unit(self, k):
        if self.use_sleep:
            self.torch.cuda._sleep(int(k))
        else:
            b = self.a
            for _ in range(int(k)):
                b = b @ self.a

    def queue(self, stream, ms):
        torch = self.torch
        with torch.cuda.stream(stream):
            self._unit(max(1, round(ms * self.units_per_ms)))
            ev = torch.cuda.Event()
            ev.record(stream)
        return ev


@contextlib.contextmanager
def no_gc():
    """No cyclic collection while a blocker is in flight: destroying a handle frees device memory,
    and that waits for the whole device, the blocker included."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def poison(a):
    """Valid values of a's dtype that differ from a: a bit is flipped (bits stay bits), a float x
    becomes 0.375 - x / 2 (finite, and different unless x is exactly 0.25)."""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return (a ^ 1).astype(np.uint8)
    if a.dtype == np.int8:
        return (a.view(np.uint8) ^ 1).view(np.int8)
    return (a * a.dtype.type(-0.5) + a.dtype.type(0.375)).astype(a.dtype)


class Ctx:
    """Where a case's work goes. `kw` is what every entry call receives ({"stream": S} or {}: torch's
    current stream); `on()` makes the stream of those calls current for the case's own torch
    operations (snapshots, masks) and for reading results back, so that they are ordered behind the
    calls and behind nothing else."""

    def __init__(self, torch, stream=None, explicit=False):
        self.torch, self.stream = torch, stream
        self.kw = {"stream": stream} if (explicit and stream is not None) else {}

    def on(self):
        return self.torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def snap(self, t):
        """A copy of t as it is at this point of the calls' stream."""
        with self.on():
            return t.clone()

    def upto(self, t, count):
        """t with everything from index count[0] on zeroed (what an entry leaves unwritten), on the device."""
        torch = self.torch
        with self.on():
            keep = torch.arange(t.shape[0], device=t.device) < count[0]
            return torch.where(keep, t, torch.zeros_like(t))

    def read(self, outs):
        """The bytes of every output, read on the calls' stream (waits for that stream alone)."""
        with self.on():
            return [o.cpu().numpy().tobytes() for o in outs]


def drive(gen):
    """Run a case's calls to the end; returns the host time they took."""
    t0 = time.perf_counter()
    for _ in gen:
        pass
    return time.perf_counter() - t0


def interleave(g1, g2):
    """A1, B1, A2, B2, ...: one call of each generator in turn until both end."""
    live = [g1, g2]
    while live:
        for g in list(live):
            try:
                next(g)
            except StopIteration:
                live.remove(g)
