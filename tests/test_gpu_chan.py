"""Channel model on the device against the float64 restatement of tests/chan_ref.py, and the
error counter against numpy.

Parity bound per component, with r = sqrt(-ln u1) and |x| the complex modulus (u = 2^-24):
    |got - ref| <= 2^-20 (|gain| |x[n]| + sqrt(n0) r[n]) + 1e-30
The angle from the top 32 bits rounded to f32 gives at most 3.1 u |x|, sin/cos about 2 u, the
products, the sum and the gain about 3 u; the noise term carries log, sqrt and sin/cos of exact
inputs, about 6 u r; 16 u leaves margin for either FMA contraction choice. f16 output adds its
rounding, 2^-11 |ref| + 2^-25. The worst ratio of every case goes to profiles/chan_margins.txt when
CHAN_MARGINS_OUT names a file."""
import os

import numpy as np
import pytest

import chan_ref

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 63, 64, 65, 255, 257, 4099]
NMAX = max(SIZES)
NP_DT = {0: np.float32, 1: np.float16}
CASES = {
    "noise": dict(n0=0.35, seed=99),
    "rot": dict(cfo=0.1234567, phase=-2.5),
    "both": dict(gain=0.37, cfo=0.1234567, phase=-2.5, n0=0.35, seed=99),
}
MARGINS = []


@pytest.fixture(scope="module")
def scatter():
    """Seeded Gaussian scatter of amplitude about 1, a few samples at 1e-3 and at 1e3."""
    rng = np.random.RandomState(20240)
    x = (rng.randn(NMAX + 1, 2) * np.sqrt(0.5)).astype(np.float32)
    x[[0, 5, 70, 300, 4098]] *= np.float32(1e-3)
    x[[2, 66, 256, 4000]] *= np.float32(1e3)
    return x


@pytest.fixture(scope="module", autouse=True)
def margins_file():
    yield
    path = os.environ.get("CHAN_MARGINS_OUT")
    if path and MARGINS:
        with open(path, "w") as f:
            f.write("# worst |got - ref| / bound per case (tests/test_gpu_chan.py); bound = 2^-20 (|gain||x| + sqrt(n0) r) + 1e-30\n"
                    "# (+ 2^-11 |ref| + 2^-25 for f16 output)\n")
            for line in MARGINS:
                f.write(line + "\n")


def bound(x, r, gain, n0, ref, out_dtype):
    mod = np.hypot(x[:, 0].astype(np.float64), x[:, 1].astype(np.float64))
    b = 2.0 ** -20 * (abs(float(np.float32(gain))) * mod + float(np.float32(np.sqrt(n0))) * r) + 1e-30
    b = np.repeat(b[:, None], 2, 1)
    if out_dtype == 1:
        b = b + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
    return b


def run_parity(m, torch, x, kw, s0, in_dtype, out_dtype, tag, offset=0, rotate=chan_ref.rotate):
    """x: float32 scatter; the kernel reads x[offset:] as in_dtype from a buffer whose start is
    16-byte aligned (offset 1: 8-byte but not 16-byte aligned for f32). `rotate`: chan_ref.rotate_np
    for millions of samples (tests/test_chan_host.py holds it equal to chan_ref.rotate)."""
    xin = x.astype(NP_DT[in_dtype])
    dev = torch.from_numpy(xin).cuda()
    assert dev.data_ptr() % 16 == 0
    ch = m.Channel(s0=s0, in_dtype=in_dtype, out_dtype=out_dtype, **kw)
    got = ch.process(dev[offset:]).cpu().numpy().astype(np.float64)
    assert ch.sample == s0 + len(x) - offset
    ref, r = chan_ref.channel(xin[offset:], gain=kw.get("gain", 1.0), nco=ch.nco, n0=kw.get("n0", 0.0),
                              seed=kw.get("seed", 0), s0=s0, rotate=rotate)
    b = bound(xin[offset:], r, kw.get("gain", 1.0), kw.get("n0", 0.0), ref, out_dtype)
    ratio = float((np.abs(got - ref) / b).max())
    line = f"{tag:44s} n {len(x) - offset:5d}  worst ratio {ratio:.3f}"
    print(line)
    MARGINS.append(line)
    assert ratio <= 1.0, line
    return got


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", list(CASES))
def test_parity_f32(m, torch_cuda, scatter, case, n):
    run_parity(m, torch_cuda, scatter[:n], CASES[case], 0, 0, 0, f"{case} f32->f32 s0 0")


@pytest.mark.parametrize("s0", [1, (1 << 40) + 3])
@pytest.mark.parametrize("case", list(CASES))
def test_parity_far_from_the_origin(m, torch_cuda, scatter, case, s0):
    for n in (65, 4099):
        run_parity(m, torch_cuda, scatter[:n], CASES[case], s0, 0, 0, f"{case} f32->f32 s0 {s0}")


@pytest.mark.parametrize("in_dtype,out_dtype", [(0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("case", list(CASES))
def test_parity_dtype_pairs(m, torch_cuda, scatter, case, in_dtype, out_dtype):
    names = {0: "f32", 1: "f16"}
    for n in (3, 257, 4099):
        run_parity(m, torch_cuda, scatter[:n], CASES[case], (1 << 40) + 3, in_dtype, out_dtype,
                   f"{case} {names[in_dtype]}->{names[out_dtype]} s0 2^40+3")


@pytest.mark.parametrize("in_dtype", [0, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_parity_narrow_path(m, torch_cuda, scatter, case, in_dtype):
    """The input starts one sample into an aligned buffer: 8-byte (f32) or 4-byte (f16) aligned, not 16."""
    for n in (4, 66, 4100):
        run_parity(m, torch_cuda, scatter[:n], CASES[case], 7, in_dtype, in_dtype,
                   f"{case} {'f32' if in_dtype == 0 else 'f16'} offset by one sample", offset=1)


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("in_dtype,out_dtype", [(0, 0), (1, 1), (0, 1), (1, 0)])
def test_cuts_give_identical_bytes(m, torch_cuda, scatter, in_dtype, out_dtype):
    torch = torch_cuda
    kw = dict(CASES["both"], s0=(1 << 40) + 3, in_dtype=in_dtype, out_dtype=out_dtype)
    x = torch.from_numpy(scatter[:4099].astype(NP_DT[in_dtype])).cuda()
    one = m.Channel(**kw)
    whole = one.process(x)
    cut = m.Channel(**kw)
    parts, prev = [], 0
    for c in [0, 1, 63, 64, 65, 4098, 4099]:
        parts.append(cut.process(x[prev:c].contiguous()))
        parts.append(cut.process(x[c:c]))                                  # a zero-length call in between
        prev = c
    assert _bytes(torch.cat(parts)) == _bytes(whole)
    assert cut.sample == one.sample == (1 << 40) + 3 + 4099
    # views into one buffer (cuts at unaligned addresses: the narrow path) give the same bytes too
    cut2 = m.Channel(**kw)
    parts = [cut2.process(x[a:b]) for a, b in ((0, 1), (1, 63), (63, 64), (64, 65), (65, 4098), (4098, 4099))]
    assert _bytes(torch.cat(parts)) == _bytes(whole)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("offset", [0, 1])
def test_in_place_equals_out_of_place(m, torch_cuda, scatter, dtype, offset):
    torch = torch_cuda
    kw = dict(CASES["both"], s0=5, in_dtype=dtype, out_dtype=dtype)
    x = torch.from_numpy(scatter[:4099].astype(NP_DT[dtype])).cuda()
    want = m.Channel(**kw).process(x[offset:])
    buf = x.clone()
    got = m.Channel(**kw).process(buf[offset:], out=buf[offset:])
    assert got.data_ptr() == buf[offset:].data_ptr()
    assert _bytes(got) == _bytes(want)
    with pytest.raises(m.ModemPanic):                                      # a shifted overlap is refused
        m.Channel(**kw).process(buf[0:100], out=buf[1:101])


def test_set_n0_between_calls(m, torch_cuda, scatter):
    torch = torch_cuda
    x = torch.from_numpy(scatter[:4099]).cuda()
    kw = dict(gain=0.37, cfo=0.1234567, phase=-2.5, seed=99)
    ch = m.Channel(n0=0.35, s0=11, **kw)
    a = ch.process(x[:1000])
    ch.set_n0(0.02)
    b = ch.process(x[1000:])
    assert _bytes(a) == _bytes(m.Channel(n0=0.35, s0=11, **kw).process(x[:1000]))
    assert _bytes(b) == _bytes(m.Channel(n0=0.02, s0=1011, **kw).process(x[1000:]))
    ch.set_n0(0.0)                                                         # and off again: no noise at all
    c = ch.process(x[:64])
    assert _bytes(c) == _bytes(m.Channel(n0=0.0, s0=11 + 4099, **kw).process(x[:64]))


def test_seeds(m, torch_cuda, scatter):
    x = torch_cuda.from_numpy(scatter[:4099]).cuda()
    a = m.Channel(n0=0.5, seed=1).process(x)
    b = m.Channel(n0=0.5, seed=1).process(x)
    c = m.Channel(n0=0.5, seed=2).process(x)
    assert _bytes(a) == _bytes(b)
    d = (a - c).cpu().numpy()
    assert np.count_nonzero(d) > 0.99 * d.size
    # another seed is another stream, not a shifted one
    assert abs(np.corrcoef((a - x).cpu().numpy()[:, 0], (c - x).cpu().numpy()[:, 0])[0, 1]) < 0.1


@pytest.mark.parametrize("dtype", [0, 1])
def test_identity(m, torch_cuda, scatter, dtype):
    xin = scatter[:4099].astype(NP_DT[dtype])
    xin[7] = (-0.0, 0.0)
    for offset in (0, 1):
        got = m.Channel(in_dtype=dtype, out_dtype=dtype, s0=123).process(torch_cuda.from_numpy(xin).cuda()[offset:])
        assert np.array_equal(got.cpu().numpy(), xin[offset:])             # as values: -0 == +0
    host = m.Channel(in_dtype=dtype, out_dtype=dtype).process(xin)         # numpy in, numpy out
    assert isinstance(host, np.ndarray) and np.array_equal(host, xin)


def test_host_buffers_equal_device_buffers(m, torch_cuda, scatter):
    kw = dict(CASES["both"], s0=9)
    x = scatter[:257]
    dev = m.Channel(**kw).process(torch_cuda.from_numpy(x).cuda()).cpu().numpy()
    host = m.Channel(**kw).process(x)
    assert isinstance(host, np.ndarray) and host.tobytes() == dev.tobytes()
    inplace = x.copy()
    m.Channel(**kw).process(inplace, out=inplace)
    assert inplace.tobytes() == dev.tobytes()


# -------------------------------------------------------------------- count_errors ----
def _pattern(n, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, n).astype(np.uint8)
    flip = np.zeros(n, np.uint8)
    idx = rng.rand(n) < 0.3
    flip[idx] = rng.randint(1, 256, int(idx.sum())).astype(np.uint8)
    if n:
        flip[-1] = 0x81                                                    # the last byte always differs, by 2 bits
    return a, a ^ flip, int(np.count_nonzero(flip)), int(np.unpackbits(flip).sum())


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4099])
def test_count_errors_against_numpy(m, torch_cuda, n):
    torch = torch_cuda
    a, b, nbytes, nbits = _pattern(n, n + 1)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    c = m.count_errors(da, db)
    assert c.dtype == torch.int64 and c.is_cuda and c.tolist() == [nbytes, nbits]
    m.count_errors(da, db, counts=c)                                       # accumulates, never clears
    a2, b2, nbytes2, nbits2 = _pattern(33, 5)
    m.count_errors(torch.from_numpy(a2).cuda(), torch.from_numpy(b2).cuda(), counts=c)
    assert c.tolist() == [2 * nbytes + nbytes2, 2 * nbits + nbits2]
    h = m.count_errors(a, b)                                               # host arrays
    assert isinstance(h, np.ndarray) and h.dtype == np.int64 and h.tolist() == [nbytes, nbits]


@pytest.mark.parametrize("oa,ob", [(1, 1), (3, 3), (1, 2), (0, 5), (15, 15)])
def test_count_errors_unaligned(m, torch_cuda, oa, ob):
    torch = torch_cuda
    n = 4099
    a, b, nbytes, nbits = _pattern(n, 17)
    da, db = torch.zeros(n + 16, dtype=torch.uint8).cuda(), torch.zeros(n + 16, dtype=torch.uint8).cuda()
    da[oa:oa + n] = torch.from_numpy(a).cuda()
    db[ob:ob + n] = torch.from_numpy(b).cuda()
    assert m.count_errors(da[oa:oa + n], db[ob:ob + n]).tolist() == [nbytes, nbits]


def test_count_errors_refusals_on_the_device(m, torch_cuda):
    torch = torch_cuda
    L = m.load_library()
    a = torch.zeros(64, dtype=torch.uint8).cuda()
    c = torch.zeros(4, dtype=torch.int64).cuda()
    host = np.zeros(64, np.uint8)
    hc = np.zeros(2, np.int64)
    E = m.ERR_INVALID_ARG
    assert L.modem_count_errors(a.data_ptr(), host.ctypes.data, 64, c.data_ptr(), 0, None) == E     # a mix
    assert L.modem_count_errors(host.ctypes.data, a.data_ptr(), 64, c.data_ptr(), 0, None) == E
    assert L.modem_count_errors(a.data_ptr(), a.data_ptr(), 64, hc.ctypes.data, 0, None) == E
    assert L.modem_count_errors(host.ctypes.data, host.ctypes.data, 64, c.data_ptr(), 0, None) == E
    assert L.modem_count_errors(a.data_ptr(), a.data_ptr(), 64, c.data_ptr() + 4, 0, None) == E     # counts misaligned
    assert L.modem_count_errors(a.data_ptr(), a.data_ptr(), 64, None, 0, None) == E
    with pytest.raises(m.ModemPanic):
        m.count_errors(a, host)
    torch.cuda.synchronize()
    assert c.tolist() == [0, 0, 0, 0] and hc.tolist() == [0, 0]
