"""Carrier synchronizer on the device against the restatement of tests/sync_ref.py.

Inputs: seeded symbols of the constellation, rotated by cfo = 0.3 pi / (M B) per symbol and a phase
of 0.3 rad, with noise at Eb/N0 = 12 dB; the tracker starts at phase0 = 0.25 rad. On the reference
every block has q_b >= 0.3 and an unwrap margin 0.5 - |wrap(Phi_b - Phi_{b-1})| >= 0.1 turn (asserted
here), so no f32 rounding can move a block to another branch.

Bounds (u = 2^-24):
  Phi_b    (2^-18 / q_b) / (2 pi) + 2^-22 turns from the float64 angle. The power costs about 3 M u
           per term, the summation (<= 16 serial and 8 tree levels) at most 24 u, both relative to
           S_b: under 64 u S_b = 2^-18 S_b on P_b, an angle of 2^-18 / q_b radians; plus the bound
           of sync_atan2_turn. The device's Phi_b is recovered exactly from theta_b: its low 32 bits
           are those of -ref, and M theta_b is Phi_b up to the few units the shifts dropped.
  quality  2^-18 from the float64 value.
  theta    equal to the integer recurrence run on the device's own Phi.
  out      2^-20 |r| from the float64 rotation by the device's own integers (the channel's
           rotation bound); f16 output adds its storage, 2^-10 |r|.
The worst ratio of every case goes to the file SYNC_MARGINS_OUT names (profiles/sync_margins.txt)."""
import ctypes
import os

import numpy as np
import pytest

import sync_ref

pytestmark = pytest.mark.gpu

NP_DT = {0: np.float32, 1: np.float16}
PHASE, PHASE0, EBN0_DB = 0.3, 0.25, 12.0
CASES = {
    "bpsk": (lambda m: m.BPSK(0.7853982, 1.0), 2, 64, 5 * 64 + 17),
    "qpsk": (lambda m: m.QPSK(0.0, 1.0), 4, 256, 3 * 256 + 1),
    "qam16": (lambda m: m.QAM(4, 0.0, 1.0), 4, 256, 4 * 256),
    "8psk": (lambda m: m.MPSK(3, 0.0, 1.0), 8, 4096, 2 * 4096 + 5),
}
MARGINS = []


@pytest.fixture(scope="module", autouse=True)
def margins_file():
    yield
    path = os.environ.get("SYNC_MARGINS_OUT")
    if path and MARGINS:
        with open(path, "w") as f:
            f.write("# worst observed error / bound per case (tests/test_gpu_sync.py): Phi (2^-18 / q_b) / (2 pi) + 2^-22 turns,\n"
                    "# quality 2^-18, out 2^-20 |r| (+ 2^-10 |r| for f16 output); theta is exact\n")
            for line in MARGINS:
                f.write(line + "\n")


_STREAMS = {}


def stream(m, name, block=None, nsym=None):
    """(x float32 (n, 2), power, block): computed once per case and shared, never modified."""
    make, power, b, n = CASES[name]
    block, nsym = block or b, nsym or n
    key = (name, block, nsym)
    if key not in _STREAMS:
        lut = make(m).lut().astype(np.float64)
        rng = np.random.RandomState(len(name) * 1000 + block)
        z = (lut[:, 0] + 1j * lut[:, 1])[rng.randint(0, len(lut), nsym)]
        n0 = sync_ref.loop_n0(lut, EBN0_DB)
        cfo = 0.3 * np.pi / (power * block)
        z = z * np.exp(1j * (PHASE + cfo * np.arange(nsym))) + np.sqrt(n0 / 2) * (rng.randn(nsym) + 1j * rng.randn(nsym))
        x = np.stack([z.real, z.imag], 1).astype(np.float32)
        x.setflags(write=False)
        _STREAMS[key] = (x, power, block)
    return _STREAMS[key]


def make_sync(m, name, block, **kw):
    return CASES[name][0](m).synchronizer(block=block, phase0=PHASE0, **kw)


def device_phi(theta, power, ref):
    """The device's Phi_b, exactly, from its theta_b (module docstring)."""
    low = (-ref) & 0xFFFFFFFF
    out = []
    for t in theta:
        turn32 = (((power * t + ref) & sync_ref.MASK) + (1 << 31) >> 32) & 0xFFFFFFFF
        out.append(((turn32 << 32) - ref) & sync_ref.MASK)
        assert out[-1] & 0xFFFFFFFF == low
    return out


def theta_ints(theta):
    return [int(v) & sync_ref.MASK for v in theta.cpu().numpy().astype(np.int64).view(np.uint64)]


def out_bound(x, out_dtype):
    mod = np.hypot(x[:, 0].astype(np.float64), x[:, 1].astype(np.float64))
    b = 2.0 ** -20 * mod + 1e-30
    if out_dtype == 1:
        b = b + 2.0 ** -10 * mod + 2.0 ** -25
    return np.repeat(b[:, None], 2, 1)


def run_parity(m, torch, name, in_dtype, out_dtype, flat=False, block=None, nsym=None, fast=False):
    """`block`, `nsym`: another shape of the case's stream. `fast`: the vectorised restatement
    (tests/test_sync_host.py holds it equal to the one used otherwise), for millions of symbols."""
    sync_fn, phases_fn, derotate_fn, top32_fn = ((sync_ref.sync_np, sync_ref.phases_np, sync_ref.derotate_np, sync_ref.top32_np) if fast else
                                                 (sync_ref.sync, sync_ref.phases, sync_ref.derotate, sync_ref.top32))
    x32, power, block = stream(m, name, block, nsym)
    xin = x32.astype(NP_DT[in_dtype])
    sy = make_sync(m, name, block, in_dtype=in_dtype, out_dtype=out_dtype, flags=m.SYNC_FLAT if flat else 0)
    assert sy.power == power
    ref, phase0 = sync_ref.turns(m, sy.ref_phase), sync_ref.turns(m, PHASE0)
    want = sync_fn(xin, power, block, sy.norm, ref, phase0, flat)
    nb = len(xin) // block
    assert want["q"].min() >= 0.3 and min(want["margins"]) >= 0.1          # the inputs keep clear of every branch cut
    out, theta, q = sy.process(torch.from_numpy(xin).cuda())
    rest = sy.flush(like=out)
    assert out.shape == (nb * block, 2) and theta.shape == (nb,) and q.shape == (nb,) and rest.shape == (len(xin) - nb * block, 2)
    assert sy.symbol == len(xin)
    th = theta_ints(theta)
    # Phi and quality against float64
    phi = device_phi(th, power, ref)
    d = np.array([((p + ref) & sync_ref.MASK) / 2.0 ** 64 for p in phi]) - want["turn"]
    d = np.abs(d - np.round(d))
    r_phi = float((d / ((2.0 ** -18 / want["q"]) / (2 * np.pi) + 2.0 ** -22)).max())
    r_q = float((np.abs(q.cpu().numpy().astype(np.float64) - want["q"]) / 2.0 ** -18).max())
    # theta: the integer recurrence on the device's own Phi
    assert sync_ref.unwrap(phi, power, phase0)[0] == th
    # out: the float64 rotation by the device's own integers
    got = np.concatenate([out.cpu().numpy(), rest.cpu().numpy()]).astype(np.float64)
    ph = phases_fn(th, block, phase0, flat, len(xin) - nb * block)
    rot = derotate_fn(xin, top32_fn(ph))
    r_out = float((np.abs(got - rot) / out_bound(xin, out_dtype)).max())
    assert np.all(np.isfinite(got))
    names = {0: "f32", 1: "f16"}
    line = (f"{name:6s} M {power} B {block:4d} n {len(xin):5d} {names[in_dtype]}->{names[out_dtype]}{' flat' if flat else ''}: "
            f"Phi {r_phi:.3f}  quality {r_q:.3f}  out {r_out:.3f}  (worst error / bound)")
    print(line)
    MARGINS.append(line)
    assert r_phi <= 1.0 and r_q <= 1.0 and r_out <= 1.0, line
    return want, th, got, xin


@pytest.mark.parametrize("name", list(CASES))
def test_parity(m, torch_cuda, name):
    run_parity(m, torch_cuda, name, 0, 0)


@pytest.mark.parametrize("in_dtype,out_dtype", [(0, 1), (1, 0), (1, 1)])
def test_parity_dtype_pairs(m, torch_cuda, in_dtype, out_dtype):
    run_parity(m, torch_cuda, "qpsk", in_dtype, out_dtype)


def test_flat_keeps_one_phase_per_block(m, torch_cuda):
    """MODEM_SYNC_FLAT: every symbol of block b is rotated by theta_b; the sloped line would miss the bound."""
    want, th, got, xin = run_parity(m, torch_cuda, "qpsk", 0, 0, flat=True)
    block = CASES["qpsk"][2]
    nb = len(th)
    ph = [t for t in th for _ in range(block)]
    const = sync_ref.derotate(xin[: nb * block], sync_ref.top32(ph))
    assert (np.abs(got[: nb * block] - const) / out_bound(xin[: nb * block], 0)).max() <= 1.0
    sloped = sync_ref.derotate(xin[: nb * block], sync_ref.phases(th, block, 0, False))
    assert (np.abs(sloped - const) / out_bound(xin[: nb * block], 0)).max() > 100.0


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _view(torch, a, how):
    """A device copy of the (n, 2) array `a`: aligned, one symbol or one element into its buffer."""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if how == "aligned":
        return t
    skip = 2 if how == "symbol" else 1
    buf = torch.zeros(t.numel() + skip, dtype=t.dtype, device=t.device)
    v = buf[skip:].view(-1, 2)
    v.copy_(t)
    return v


@pytest.mark.parametrize("how", ["aligned", "symbol", "element"])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("block", [64, 256])
def test_cuts_give_identical_bytes(m, torch_cuda, block, dtype, how):
    torch = torch_cuda
    n = 3 * block + 37
    x32, power, _ = stream(m, "qpsk", block, n)
    xin = x32.astype(NP_DT[dtype])
    kw = dict(in_dtype=dtype, out_dtype=dtype)
    one = make_sync(m, "qpsk", block, **kw)
    out1, th1, q1 = one.process(torch.from_numpy(xin).cuda())
    rest1 = one.flush(like=out1)
    assert out1.shape[0] == 3 * block and rest1.shape[0] == 37
    cut = make_sync(m, "qpsk", block, **kw)
    outs, ths, qs, prev = [], [], [], 0
    for c in [0, 1, block - 1, block, block + 1, 2 * block - 1, n]:
        for a, b in ((prev, c), (c, c)):                                   # the piece, then a zero-length call
            src = _view(torch, xin[a:b], how)
            dst = _view(torch, np.zeros((cut.nblocks(b - a) * block, 2), NP_DT[dtype]), how)
            o, t, q = cut.process(src, out=dst)
            assert o.shape[0] == dst.shape[0]
            outs.append(o); ths.append(t); qs.append(q)
        prev = c
    rest = _view(torch, np.zeros((37, 2), NP_DT[dtype]), how)
    got = ctypes.c_size_t()
    assert m.load_library().modem_sync_flush(cut._h, rest.data_ptr(), 37, ctypes.byref(got), None) == m.MODEM_OK
    torch.cuda.synchronize()
    assert got.value == 37 and cut.symbol == one.symbol == n
    assert _bytes(torch.cat(outs)) == _bytes(out1)
    assert _bytes(torch.cat(ths)) == _bytes(th1) and _bytes(torch.cat(qs)) == _bytes(q1)
    assert _bytes(rest) == _bytes(rest1)


def test_host_buffers_equal_device_buffers(m, torch_cuda):
    x32, power, block = stream(m, "qpsk")
    dev = make_sync(m, "qpsk", block)
    out, theta, q = dev.process(torch_cuda.from_numpy(np.array(x32)).cuda())
    host = make_sync(m, "qpsk", block)
    hout, htheta, hq = host.process(np.array(x32))
    assert isinstance(hout, np.ndarray) and htheta.dtype == np.uint64
    assert hout.tobytes() == _bytes(out) and htheta.tobytes() == _bytes(theta) and hq.tobytes() == _bytes(q)
    assert host.flush().tobytes() == _bytes(dev.flush(like=out))


def test_a_stream_shorter_than_a_block(m, torch_cuda):
    """process emits nothing; flush rotates by phase0 (no block was ever completed)."""
    x32, power, block = stream(m, "qpsk")
    x = x32[:100]
    sy = make_sync(m, "qpsk", block)
    out, theta, q = sy.process(torch_cuda.from_numpy(np.array(x[:60])).cuda())
    assert out.shape == (0, 2) and theta.shape == (0,) and q.shape == (0,)
    out, theta, q = sy.process(torch_cuda.from_numpy(np.array(x[60:])).cuda())
    assert out.shape == (0, 2) and sy.symbol == 100
    rest = sy.flush(like=out)
    assert rest.shape == (100, 2)
    p0 = sync_ref.turns(m, PHASE0)
    want = sync_ref.derotate(x, sync_ref.top32([p0] * 100))
    assert (np.abs(rest.cpu().numpy().astype(np.float64) - want) / out_bound(x, 0)).max() <= 1.0
    assert sy.flush(like=out).shape == (0, 2)                              # at a block boundary now


def test_refusals_leave_the_state_and_the_output(m, torch_cuda):
    torch = torch_cuda
    L = m.load_library()
    x32, power, block = stream(m, "qpsk")
    x = torch.from_numpy(np.array(x32)).cuda()
    n = x.shape[0]
    sy = make_sync(m, "qpsk", block)
    sy.process(x[:10])                                                      # 10 carried symbols
    out = torch.full((n + 16, 2), 7.0, dtype=torch.float32, device=x.device)
    theta = torch.full((8,), 7, dtype=torch.int64, device=x.device)
    q = torch.full((8,), 7.0, dtype=torch.float32, device=x.device)
    prod, blocks = ctypes.c_size_t(5), ctypes.c_size_t(5)
    args = (ctypes.byref(prod), ctypes.byref(blocks), None)
    nb = (10 + n) // block
    assert L.modem_sync_process(sy._h, x.data_ptr(), n, out.data_ptr(), nb * block - 1, theta.data_ptr(), q.data_ptr(), 8, *args) == m.ERR_CAPACITY
    assert prod.value == 0 and blocks.value == 0
    assert L.modem_sync_process(sy._h, x.data_ptr(), n, out.data_ptr(), n + 16, theta.data_ptr(), q.data_ptr(), nb - 1, *args) == m.ERR_CAPACITY
    assert L.modem_sync_process(sy._h, x.data_ptr(), n, out.data_ptr(), n + 16, None, q.data_ptr(), nb - 1, *args) == m.ERR_CAPACITY
    assert L.modem_sync_flush(sy._h, out.data_ptr(), 9, None, None) == m.ERR_CAPACITY
    # overlapping input and output ranges: the same address, and a shifted one
    assert L.modem_sync_process(sy._h, x.data_ptr(), n, x.data_ptr(), n, None, None, 0, *args) == m.ERR_INVALID_ARG
    assert L.modem_sync_process(sy._h, x.data_ptr(), n, x.data_ptr() + 8 * (n - 1), n, None, None, 0, *args) == m.ERR_INVALID_ARG
    assert L.modem_sync_process(sy._h, x.data_ptr() + 8, n - 1, x.data_ptr(), n, None, None, 0, *args) == m.ERR_INVALID_ARG
    assert L.modem_sync_process(sy._h, None, 1, out.data_ptr(), n, None, None, 0, *args) == m.ERR_INVALID_ARG
    assert L.modem_sync_process(sy._h, x.data_ptr(), n, None, n, None, None, 0, *args) == m.ERR_INVALID_ARG      # NULL out
    torch.cuda.synchronize()
    assert sy.symbol == 10
    assert bool((out == 7.0).all()) and bool((theta == 7).all()) and bool((q == 7.0).all())
    assert _bytes(x) == x32.tobytes()
    # the handle goes on as if nothing had been asked
    fresh = make_sync(m, "qpsk", block)
    fresh.process(x[:10])
    a, b = sy.process(x), fresh.process(x)
    assert all(_bytes(u) == _bytes(v) for u, v in zip(a, b)) and a[0].shape[0] == nb * block


def test_an_all_zero_block(m, torch_cuda):
    """q = 0, Phi = -ref, and the output stays finite (a fade, or the gap between two bursts)."""
    x32, power, block = stream(m, "qpsk")
    x = np.array(x32[: 3 * block])
    x[block: 2 * block] = 0.0
    sy = make_sync(m, "qpsk", block)
    ref = sync_ref.turns(m, sy.ref_phase)
    out, theta, q = sy.process(torch_cuda.from_numpy(x).cuda())
    th = theta_ints(theta)
    phi = device_phi(th, power, ref)
    assert float(q[1]) == 0.0 and float(q[0]) > 0.3 and float(q[2]) > 0.3
    assert phi[1] == (-ref) & sync_ref.MASK
    assert sync_ref.unwrap(phi, power, sync_ref.turns(m, PHASE0))[0] == th
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got)) and not got[block: 2 * block].any()
