"""Symbol timing synchronizer on the device against the restatement of tests/timing_ref.py.

Inputs (timing_ref.case_stream): QPSK through a raised cosine of roll-off 0.5, the delay 0.3 symbol
at the start and drifting by 0.2 symbol per block, white noise at Eb/N0 = 12 dB; the tracker starts
0.1 symbol away. On the restatement every block has q_b >= 0.02 and an unwrap margin
0.5 - |wrap| / 2^32 >= 0.1 symbol (asserted here), so no f32 rounding can move a block to another
branch.

Bounds (u = 2^-24), from the summation order and the coefficient arithmetic the header states:
  Phi_b    (c u / q_b) / (2 pi) + 2^-22 symbol from the float64 angle. A term fma(re, re, im*im)
           is within 2 u of |x|^2; the terms are not negative, so a sum of depth d is within d u of
           exact, relative: an accumulator adds B N / 512 rows, the join of four costs 2, the tree 4
           levels (5 when N = 4). X is made of differences of the E_p (1 more), for N = 8 also the
           rounded h, its product and two more sums (4 more); all relative to parts of S_b. Hence
           |X_dev - X| <= c u S_b with c = 2 + max(1, B N / 512) + 2 + (4 | 5) + 1 (+ 4) =
           timing_ref.line_c, an angle of c u / q_b radians; plus the bound of the 32-bit angle.
           The device's Phi_b is the low 32 bits of tau[b].
  quality  (2 c + 6) u: |X| moved by c u S and rounded 4 times, S by its own summation, one division.
  tau      equal to the integer recurrence run on the device's own Phi.
  out      12 u max|tap| per component against the float64 interpolation at the device's own
           integers: a = mu + 1 and d = mu - 2 round once, b = mu - 1 is exact, so a coefficient
           carries at most 5 u (two rounded factors or one and the rounded 1/6, two products, one
           scaling); sum |c_j| <= 1.25, so the coefficients cost 6.25 u max|tap|, and the product
           and the three fused adds at most u each on partial sums below 1.25 max|tap|: 5 u more.
           F16 output adds its storage, 2^-11 |out| + 2^-25.
The worst ratio of every case goes to the file TIMING_MARGINS_OUT names (profiles/timing_margins.txt)."""
import ctypes
import os

import numpy as np
import pytest

import timing_ref as R

pytestmark = pytest.mark.gpu

NP_DT = {0: np.float32, 1: np.float16}
NAMES = {0: "f32", 1: "f16"}
MARGINS = []


@pytest.fixture(scope="module", autouse=True)
def margins_file():
    yield
    path = os.environ.get("TIMING_MARGINS_OUT")
    if path and MARGINS:
        with open(path, "w") as f:
            f.write("# worst observed error / bound per case (tests/test_gpu_timing.py): Phi (c u / q_b) / (2 pi) + 2^-22 symbol,\n"
                    "# quality (2 c + 6) u, out 12 u max|tap| (+ 2^-11 |out| for f16 output); tau is exact\n")
            for line in MARGINS:
                f.write(line + "\n")


def tau_ints(tau):
    return [int(v) for v in tau.cpu().numpy()]


def out_bound(taps, want, out_dtype):
    """(n, 2): per component, from the (n, 4) complex taps and the float64 result."""
    big = np.stack([np.abs(taps.real).max(1), np.abs(taps.imag).max(1)], 1)
    b = R.OUT_C * R.U * big + 1e-37
    if out_dtype == 1:
        b = b + 2.0 ** -11 * np.abs(R.pairs(want)) + 2.0 ** -25
    return b


def check(m, torch, x, sps, block, span, tau0, in_dtype, out_dtype, flat=False, label="", fast=False):
    """One stream through process and flush, held against the restatement. Returns (want, D, got).
    `fast`: the vectorised restatement (tests/test_timing_host.py holds it equal to the one used
    otherwise), for millions of samples."""
    timing_fn, positions_fn = (R.timing_np, R.positions_np) if fast else (R.timing, R.positions)
    xin = np.asarray(x).astype(NP_DT[in_dtype])
    z = R.cplx(xin)
    want = timing_fn(z, sps, block, span, tau0, flat)
    ts = m.TimingSync(sps, block=block, span=span, tau0=tau0, flat=flat, in_dtype=in_dtype, out_dtype=out_dtype)
    out, tau, q = ts.process(torch.from_numpy(xin).cuda())
    rest = ts.flush(like=out)
    nb = len(xin) // (block * sps)
    nfl = (len(xin) - nb * block * sps) // sps
    assert out.shape == (nb * block, 2) and tau.shape == (nb,) and q.shape == (nb,) and rest.shape == (nfl, 2)
    assert ts.sample == len(xin)
    D = tau_ints(tau)
    phi = [d & 0xFFFFFFFF for d in D]
    assert R.unwrap(phi, R.d_start(tau0))[0] == D                      # tau: the recurrence on the device's own Phi
    qd = q.cpu().numpy().astype(np.float64)
    mpos, mu24 = positions_fn(D, R.d_start(tau0), sps, block, span, flat, nfl)
    ref, taps = R.interpolate(z, mpos, mu24)
    got = np.concatenate([out.cpu().numpy(), rest.cpu().numpy()]).astype(np.float64)
    assert np.all(np.isfinite(got))
    r_out = float((np.abs(got - R.pairs(ref)) / out_bound(taps, ref, out_dtype)).max()) if len(got) else 0.0
    return want, D, got, qd, r_out


def run_parity(m, torch, name, in_dtype, out_dtype, flat=False, case=None, fast=False):
    """`case`: (x, sps, block) of another stream in place of R.case_stream(name); `fast` as in check()."""
    x, sps, block = case or R.case_stream(name)
    want, D, got, qd, r_out = check(m, torch, x, sps, block, R.CASE_SPAN, R.CASE_TAU0, in_dtype, out_dtype, flat, fast=fast)
    assert want["q"].min() >= 0.02 and min(want["margins"]) >= 0.1         # the inputs keep clear of every branch cut
    d = np.array([(v & 0xFFFFFFFF) / 2.0 ** 32 for v in D]) - want["turn"]
    d = np.abs(d - np.round(d))
    r_phi = float((d / R.phi_bound(want["q"], sps, block)).max())
    r_q = float((np.abs(qd - want["q"]) / R.q_bound(sps, block)).max())
    line = (f"{name:9s} N {sps} B {block:4d} n {len(x):5d} {NAMES[in_dtype]}->{NAMES[out_dtype]}{' flat' if flat else ''}: "
            f"Phi {r_phi:.3f}  quality {r_q:.3f}  out {r_out:.3f}  (worst error / bound)")
    print(line)
    MARGINS.append(line)
    assert r_phi <= 1.0 and r_q <= 1.0 and r_out <= 1.0, line
    return want, D, got


@pytest.mark.parametrize("name", list(R.CASES))
def test_parity(m, torch_cuda, name):
    run_parity(m, torch_cuda, name, 0, 0)


@pytest.mark.parametrize("in_dtype,out_dtype", [(1, 0), (0, 1)])
@pytest.mark.parametrize("name", list(R.CASES))
def test_parity_dtype_pairs(m, torch_cuda, name, in_dtype, out_dtype):
    run_parity(m, torch_cuda, name, in_dtype, out_dtype)


def test_flat_keeps_one_delay_per_block(m, torch_cuda):
    want, D, got = run_parity(m, torch_cuda, "n4_b256", 0, 0, flat=True)
    sloped = R.timing(R.cplx(R.case_stream("n4_b256")[0]), 4, 256, R.CASE_SPAN, R.CASE_TAU0, False)
    assert np.abs(R.pairs(sloped["out"]) - got).max() > 1e-3              # the line is a different output


@pytest.mark.parametrize("sps", [4, 8])
@pytest.mark.parametrize("half", [False, True])
def test_grid_aligned_streams_are_exact(m, torch_cuda, sps, half):
    """Nonzero only at n = 0 (or N/2) mod N: Phi = 0 (2^31), D = 0 (-2^31), out a bitwise copy."""
    torch = torch_cuda
    block, span, nb = 64, 2, 3
    rng = np.random.RandomState(7 + sps + half)
    x = np.zeros((nb * block * sps, 2), np.float32)
    at = sps // 2 if half else 0
    x[at::sps] = (rng.randn(nb * block, 2) + 3.0).astype(np.float32)
    ts = m.TimingSync(sps, block=block, span=span)
    out, tau, q = ts.process(torch.from_numpy(x).cuda())
    assert tau_ints(tau) == [-(1 << 31) if half else 0] * nb
    assert np.abs(q.cpu().numpy() - 1.0).max() <= 2.0 ** -22
    k = np.arange(nb * block)
    src = sps * (k - span) - at
    want = np.where((src >= 0)[:, None], x[np.clip(src, 0, None)], np.float32(0.0))
    assert out.cpu().numpy().tobytes() == want.astype(np.float32).tobytes()


def test_an_all_zero_block(m, torch_cuda):
    """q = 0, Phi = 0, and the output stays finite (a fade, or the gap between two bursts)."""
    x0, sps, block = R.case_stream("n4_b256")
    x = np.array(x0[: 3 * block * sps])
    x[block * sps: 2 * block * sps] = 0.0
    ts = m.TimingSync(sps, block=block, span=R.CASE_SPAN, tau0=R.CASE_TAU0)
    out, tau, q = ts.process(torch_cuda.from_numpy(x).cuda())
    D = tau_ints(tau)
    assert float(q[1]) == 0.0 and float(q[0]) > 0.02 and float(q[2]) > 0.02
    assert D[1] & 0xFFFFFFFF == 0
    assert R.unwrap([d & 0xFFFFFFFF for d in D], R.d_start(R.CASE_TAU0))[0] == D
    assert np.all(np.isfinite(out.cpu().numpy()))


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _view(torch, a, how):
    """A device copy of the (n, 2) array `a`: aligned, one sample or one element into its buffer."""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if how == "aligned":
        return t
    skip = 2 if how == "sample" else 1
    buf = torch.zeros(t.numel() + skip, dtype=t.dtype, device=t.device)
    v = buf[skip:].view(-1, 2)
    v.copy_(t)
    return v


@pytest.mark.parametrize("how", ["aligned", "sample", "element"])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("sps,block", [(4, 32), (8, 64)])
def test_cuts_give_identical_bytes(m, torch_cuda, sps, block, dtype, how):
    torch = torch_cuda
    bn = block * sps
    n = 3 * bn + 9 * sps + 3
    x32, _, _ = R.case_stream("n4_b32" if sps == 4 else "n8_b64", sps, block, n)
    xin = x32.astype(NP_DT[dtype])
    kw = dict(block=block, span=R.CASE_SPAN, tau0=R.CASE_TAU0, in_dtype=dtype, out_dtype=dtype)
    one = m.TimingSync(sps, **kw)
    out1, tau1, q1 = one.process(torch.from_numpy(xin).cuda())
    rest1 = one.flush(like=out1)
    assert out1.shape[0] == 3 * block and rest1.shape[0] == 9
    cut = m.TimingSync(sps, **kw)
    outs, taus, qs, prev = [], [], [], 0
    for c in [0, 1, sps + 1, bn - 1, bn, bn + 2, 2 * bn - 1, 2 * bn + sps // 2, n]:   # inside symbols, at and around block edges
        for a, b in ((prev, c), (c, c)):                                   # the piece, then a zero-length call
            src = _view(torch, xin[a:b], how)
            dst = _view(torch, np.zeros((cut.nblocks(b - a) * block, 2), NP_DT[dtype]), how)
            o, t, q = cut.process(src, out=dst)
            assert o.shape[0] == dst.shape[0]
            outs.append(o); taus.append(t); qs.append(q)
        prev = c
    rest = _view(torch, np.zeros((9, 2), NP_DT[dtype]), how)
    got = ctypes.c_size_t()
    assert m.load_library().modem_timing_flush(cut._h, rest.data_ptr(), 9, ctypes.byref(got), None) == m.MODEM_OK
    torch.cuda.synchronize()
    assert got.value == 9 and cut.sample == one.sample == n
    assert _bytes(torch.cat(outs)) == _bytes(out1)
    assert _bytes(torch.cat(taus)) == _bytes(tau1) and _bytes(torch.cat(qs)) == _bytes(q1)
    assert _bytes(rest) == _bytes(rest1)
    # after the flush both handles are at a block boundary with an all-zero history
    a, b = one.process(torch.from_numpy(xin[:bn]).cuda()), cut.process(torch.from_numpy(xin[:bn]).cuda())
    assert all(_bytes(u) == _bytes(v) for u, v in zip(a, b)) and a[0].shape[0] == block


def test_host_buffers_equal_device_buffers(m, torch_cuda):
    x32, sps, block = R.case_stream("n4_b32")
    kw = dict(block=block, span=R.CASE_SPAN, tau0=R.CASE_TAU0)
    dev = m.TimingSync(sps, **kw)
    out, tau, q = dev.process(torch_cuda.from_numpy(np.array(x32)).cuda())
    host = m.TimingSync(sps, **kw)
    hout, htau, hq = host.process(np.array(x32))
    assert isinstance(hout, np.ndarray) and htau.dtype == np.int64
    assert hout.tobytes() == _bytes(out) and htau.tobytes() == _bytes(tau) and hq.tobytes() == _bytes(q)
    assert host.flush().tobytes() == _bytes(dev.flush(like=out))


def test_a_stream_shorter_than_a_block(m, torch_cuda):
    """process emits nothing; flush interpolates at D_{-1} with s = 0 (no block was ever completed)."""
    x32, sps, block = R.case_stream("n4_b256")
    x = np.array(x32[: 100 * sps + 2])
    ts = m.TimingSync(sps, block=block, span=R.CASE_SPAN, tau0=R.CASE_TAU0)
    out, tau, q = ts.process(torch_cuda.from_numpy(x[:61]).cuda())
    assert out.shape == (0, 2) and tau.shape == (0,) and q.shape == (0,)
    out, tau, q = ts.process(torch_cuda.from_numpy(x[61:]).cuda())
    assert out.shape == (0, 2) and ts.sample == len(x)
    rest = ts.flush(like=out)
    assert rest.shape == (100, 2)
    z = R.cplx(x)
    mpos, mu24 = R.positions([], R.d_start(R.CASE_TAU0), sps, block, R.CASE_SPAN, False, 100)
    ref, taps = R.interpolate(z, mpos, mu24)
    assert (np.abs(rest.cpu().numpy().astype(np.float64) - R.pairs(ref)) / out_bound(taps, ref, 0)).max() <= 1.0
    assert np.abs(ref[R.CASE_SPAN + 1:]).min() > 0                          # the check saw signal
    assert ts.flush(like=out).shape == (0, 2)                              # at a block boundary now


def test_refusals_leave_the_state_and_the_output(m, torch_cuda):
    torch = torch_cuda
    L = m.load_library()
    x32, sps, block = R.case_stream("n4_b32")
    x = torch.from_numpy(np.array(x32)).cuda()
    n = x.shape[0]
    kw = dict(block=block, span=R.CASE_SPAN, tau0=R.CASE_TAU0)
    ts = m.TimingSync(sps, **kw)
    ts.process(x[:10])                                                      # 10 carried samples
    out = torch.full((n + 16, 2), 7.0, dtype=torch.float32, device=x.device)
    tau = torch.full((8,), 7, dtype=torch.int64, device=x.device)
    q = torch.full((8,), 7.0, dtype=torch.float32, device=x.device)
    prod, blocks = ctypes.c_size_t(5), ctypes.c_size_t(5)
    args = (ctypes.byref(prod), ctypes.byref(blocks), None)
    nb = (10 + n) // (block * sps)
    assert nb == 5
    assert L.modem_timing_process(ts._h, x.data_ptr(), n, out.data_ptr(), nb * block - 1, tau.data_ptr(), q.data_ptr(), 8, *args) == m.ERR_CAPACITY
    assert prod.value == 0 and blocks.value == 0
    assert L.modem_timing_process(ts._h, x.data_ptr(), n, out.data_ptr(), n + 16, tau.data_ptr(), q.data_ptr(), nb - 1, *args) == m.ERR_CAPACITY
    assert L.modem_timing_process(ts._h, x.data_ptr(), n, out.data_ptr(), n + 16, None, q.data_ptr(), nb - 1, *args) == m.ERR_CAPACITY
    assert L.modem_timing_flush(ts._h, out.data_ptr(), 1, None, None) == m.ERR_CAPACITY       # 10 samples carried: 2 symbols
    # overlapping input and output ranges: the same address, and shifted ones
    assert L.modem_timing_process(ts._h, x.data_ptr(), n, x.data_ptr(), n, None, None, 0, *args) == m.ERR_INVALID_ARG
    assert L.modem_timing_process(ts._h, x.data_ptr(), n, x.data_ptr() + 8 * (n - 1), n, None, None, 0, *args) == m.ERR_INVALID_ARG
    assert L.modem_timing_process(ts._h, x.data_ptr() + 8, n - 1, x.data_ptr(), n, None, None, 0, *args) == m.ERR_INVALID_ARG
    assert L.modem_timing_process(ts._h, None, 1, out.data_ptr(), n, None, None, 0, *args) == m.ERR_INVALID_ARG
    assert L.modem_timing_process(ts._h, x.data_ptr(), n, None, n, None, None, 0, *args) == m.ERR_INVALID_ARG    # NULL out
    torch.cuda.synchronize()
    assert ts.sample == 10
    assert bool((out == 7.0).all()) and bool((tau == 7).all()) and bool((q == 7.0).all())
    assert _bytes(x) == x32.tobytes()
    # the handle goes on as if nothing had been asked
    fresh = m.TimingSync(sps, **kw)
    fresh.process(x[:10])
    a, b = ts.process(x), fresh.process(x)
    assert all(_bytes(u) == _bytes(v) for u, v in zip(a, b)) and a[0].shape[0] == nb * block


def test_positions_clamp_at_the_span(m, torch_cuda):
    """The tracker starts at tau0 = span and the delay pulls beyond it: the positions clamp at
    +span as the restatement says, and tau goes on unclamped."""
    sps, block, span = 4, 32, 1
    n = 4 * block * sps
    rng = np.random.RandomState(11)
    pts = ((2 * rng.randint(0, 2, n // sps + 2) - 1) + 1j * (2 * rng.randint(0, 2, n // sps + 2) - 1)) / np.sqrt(2)
    x = R.pairs(R.stream(pts, sps, n, 1.2, 0.2 / block, 0.5)).astype(np.float32)
    want, D, got, qd, r_out = check(m, torch_cuda, x, sps, block, span, float(span), 0, 0)
    assert min(want["margins"]) >= 0.1
    assert min(D) > span << 32                                               # every block beyond the span
    mpos, mu24 = R.positions(D, R.d_start(float(span)), sps, block, span)
    k = np.arange(len(mpos))
    assert np.array_equal(mpos, sps * k) and not mu24.any()                   # e = +span: out[k] = x[N k]
    assert got.astype(np.float32).tobytes() == x[::sps].tobytes()
    assert r_out <= 1.0
