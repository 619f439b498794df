"""Calls whose pointers lie on different sides. Every stage that stages host memory is run three
times on a fresh handle with the same arguments: every buffer on the device, host input with
device outputs, device input with host outputs. Each run is two calls whose cut leaves carried
state (1001 then 2003 input elements), and the outputs of the two mixed runs must be the bytes
of the all-device run. The per-stage tests cover "all host equals all device"; these rows cover
the bookkeeping in between: what is staged, which buffer the kernel gets, what is copied back.
Then the refusals of a device pointer that is not element-aligned, and TX taking one."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CUTS = (1001, 2003)
_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}


def _put(torch, a, side):
    """The numpy array itself, or its bytes in a device tensor (unsigned 32 / 64 bits as signed)."""
    if side == "host":
        return a
    return torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype))).cuda()


def _zeros(torch, shape, dtype, side):
    return _put(torch, np.zeros(shape, dtype), side)


def _bytes(x):
    return (x if isinstance(x, np.ndarray) else x.cpu().numpy()).tobytes()


def _chunks(x):
    return x[:CUTS[0]], x[CUTS[0]:CUTS[0] + CUTS[1]]


def _iq(seed, n=sum(CUTS)):
    return np.random.RandomState(seed).standard_normal((n, 2)).astype(np.float32)


def _qpsk(seed, n=sum(CUTS)):
    """Unit QPSK points turned by a slow ramp, with a little noise."""
    rng = np.random.RandomState(seed)
    z = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.randint(0, 4, n) + 2e-3 * np.arange(n)))
    z = z + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return np.stack([z.real, z.imag], axis=1).astype(np.float32)


def _sh(m):
    return m._stream_handle(None, 0)


def _ok(m, status):
    assert status == m.MODEM_OK, m.status_str(status)


# ---- one function per entry: (m, torch, input side, output side) -> the outputs' bytes, call by call
def _tx(m, torch, si, so):
    bits = np.random.RandomState(1).randint(0, 2, sum(CUTS)).astype(np.uint8)
    tx = m.DigitalModulator(m.Carrier(m.Freq(1, 4)), m.QAM(4, 0.0, 1.0), 4, m.rrc_taps(33, 4, 0.35))
    res = []
    for b in _chunks(bits):                       # 4 bits per symbol: 1001 bits leave one carried
        out = _zeros(torch, (tx.nsamples(len(b)), 2), np.float32, so)
        y = tx.process(_put(torch, b, si), out=out)
        assert y.shape[0] == out.shape[0]
        res.append(_bytes(out))
    return res


def _rx(m, torch, si, so):
    x, qam = _iq(2), m.QAM(4, 0.0, 1.0)
    rx = m.DemodulatorRx(m.Carrier(m.Freq(1, 4)), m.rrc_taps(33, 4, 0.35), decim=4, decim_offset=32,
                         mix=m.MIX_COMPLEX, slicer=qam.slicer())
    res = []
    for c in _chunks(x):
        k = rx.noutputs(len(c))
        oiq, osym = _zeros(torch, (k, 2), np.float32, so), _zeros(torch, (k,), np.uint8, so)
        riq, rsym = rx.process(_put(torch, c, si), out_iq=oiq, out_sym=osym)
        assert riq.shape[0] == k and rsym.shape[0] == k
        res += [_bytes(oiq), _bytes(osym)]
    return res


def _fir(m, torch, si, so):
    x = _iq(3)[:, 0].copy()
    f = m.FIRFilter(m.rrc_taps(33, 4, 0.35))
    res = []
    for c in _chunks(x):
        xin, y = _put(torch, c, si), _zeros(torch, (len(c),), np.float32, so)
        _ok(m, m.load_library().modem_fir_process(f._h, m._ptr(xin), m._ptr(y), len(c), _sh(m)))
        res.append(_bytes(y))
    return res


def _demap(m, torch, si, so):
    d = m.SoftDemapper(m.QAM(4, 0.0, 1.0))
    res = []
    for c in _chunks(_iq(4)):
        out = _zeros(torch, (len(c), 4), np.float32, so)
        d.process(_put(torch, c, si), 2.0, out=out)
        res.append(_bytes(out))
    return res


def _diff(m, torch, si, so):
    d = m.DMPSK(2, 1.0, 0.0, float(np.pi / 2)).detector()
    res = []
    for c in _chunks(_iq(5)):                     # the last point of a call is carried into the next
        sym, llr = _zeros(torch, (len(c),), np.uint8, so), _zeros(torch, (len(c), 2), np.float32, so)
        d.process(_put(torch, c, si), 1.5, out_sym=sym, out_llr=llr)
        res += [_bytes(sym), _bytes(llr)]
    return res


def _fsk(m, torch, si, so):
    d = m.ToneDetector(np.array([-0.6, -0.2, 0.2, 0.6], np.float32), 8)
    res = []
    for c in _chunks(_iq(6)):                     # 8 samples per symbol: 1001 samples leave one carried
        k = d.nsymbols(len(c))
        sym, llr, en = (_zeros(torch, (k,), np.uint8, so), _zeros(torch, (k, 2), np.float32, so),
                        _zeros(torch, (k, 4), np.float32, so))
        got = d.process(_put(torch, c, si), 1.5, out_sym=sym, out_llr=llr, out_energy=en)
        assert got[0].shape[0] == k
        res += [_bytes(sym), _bytes(llr), _bytes(en)]
    return res


def _chan(m, torch, si, so):
    ch = m.Channel(gain=0.9, phase=0.3, cfo=0.01, n0=0.01, seed=7)
    res = []
    for c in _chunks(_iq(7)):
        out = _zeros(torch, (len(c), 2), np.float32, so)
        ch.process(_put(torch, c, si), out=out)
        res.append(_bytes(out))
    return res


def _blocks(m, torch, si, so, h, fn, per_block, est_dtype):
    """The two synchronizers: 64 symbols per block, the symbols and both estimates of every block."""
    res, carried = [], 0
    for c in _chunks(_qpsk(8)):
        nb = (carried + len(c)) // per_block
        carried = (carried + len(c)) % per_block
        assert nb >= 2
        xin = _put(torch, c, si)
        out, est, q = (_zeros(torch, (nb * 64, 2), np.float32, so), _zeros(torch, (nb,), est_dtype, so),
                       _zeros(torch, (nb,), np.float32, so))
        prod, blocks = ctypes.c_size_t(), ctypes.c_size_t()
        _ok(m, fn(h._h, m._ptr(xin), len(c), m._ptr(out), nb * 64, m._ptr(est), m._ptr(q), nb, ctypes.byref(prod),
                  ctypes.byref(blocks), _sh(m)))
        assert (prod.value, blocks.value) == (nb * 64, nb)
        res += [_bytes(out), _bytes(est), _bytes(q)]
    return res


def _sync(m, torch, si, so):
    return _blocks(m, torch, si, so, m.CarrierSync(4, block=64), m.load_library().modem_sync_process, 64, np.uint64)


def _timing(m, torch, si, so):
    return _blocks(m, torch, si, so, m.TimingSync(4, block=64), m.load_library().modem_timing_process, 256, np.int64)


FRAME_L, FRAME_CAP = 16, 64


def _frame_stream():
    rng = np.random.RandomState(9)
    u = rng.choice([-1.0, 1.0], (FRAME_L, 2)).astype(np.float32)
    x = rng.randint(-1, 2, (sum(CUTS), 2)).astype(np.float32)
    for s in (100, 500, 990, 1500, 2900):         # the third one straddles the cut
        x[s:s + FRAME_L] = u
    return x, u


def _frame(m, torch, si, so):
    x, u = _frame_stream()
    fs = m.FrameSync(u, guard=FRAME_L, threshold=0.9)
    res, hits = [], 0
    for c in _chunks(x):
        xin = _put(torch, c, si)
        pos, phi, met, cnt = (_zeros(torch, (FRAME_CAP,), np.uint64, so), _zeros(torch, (FRAME_CAP,), np.uint32, so),
                              _zeros(torch, (FRAME_CAP,), np.float32, so), _zeros(torch, (1,), np.uint64, so))
        _ok(m, m.load_library().modem_frame_process(fs._h, m._ptr(xin), len(c), m._ptr(pos), m._ptr(phi), m._ptr(met),
                                                    FRAME_CAP, m._ptr(cnt), _sh(m)))
        res += [_bytes(pos), _bytes(phi), _bytes(met), _bytes(cnt)]
        hits += int(np.frombuffer(res[-1], np.uint64)[0])
    assert 4 <= hits <= FRAME_CAP
    return res


def _gather(m, torch, si, so):
    """No handle and no state: one call over the whole stream, on the hits of a device run."""
    x, u = _frame_stream()
    fs = m.FrameSync(u, guard=FRAME_L, threshold=0.9)
    pos, phi, _, cnt = (t.cpu().numpy() for t in fs.process(torch.from_numpy(x).cuda(), cap=FRAME_CAP))
    assert int(cnt[0]) >= 4
    xin, pin, fin, cin = (_put(torch, a, si) for a in (x, pos, phi, cnt))
    length = 5
    out, ok = _zeros(torch, (FRAME_CAP, length, 2), np.float32, so), _zeros(torch, (FRAME_CAP,), np.uint8, so)
    _ok(m, m.load_library().modem_frame_gather(m._ptr(xin), len(x), 0, m._ptr(pin), m._ptr(fin), m._ptr(cin), FRAME_CAP,
                                               FRAME_L, length, 4, m.DTYPE_F32, m.DTYPE_F32, m._ptr(out), m._ptr(ok), 0,
                                               _sh(m)))
    return [_bytes(out), _bytes(ok)]


ROWS = {"tx": _tx, "rx": _rx, "fir": _fir, "demap": _demap, "diff": _diff, "fsk": _fsk, "chan": _chan,
        "sync": _sync, "timing": _timing, "frame": _frame, "gather": _gather}


@pytest.mark.parametrize("name", list(ROWS))
def test_mixed_sides_give_the_all_device_bytes(m, torch_cuda, name):
    row = ROWS[name]
    want = row(m, torch_cuda, "dev", "dev")
    assert any(any(w) for w in want), "the all-device run wrote nothing"
    for si, so in (("host", "dev"), ("dev", "host")):
        got = row(m, torch_cuda, si, so)
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"{name}: {si} input, {so} outputs: output {k} differs from the all-device run"


def test_misaligned_device_pointers_are_refused(m, torch_cuda):
    """A device pointer one byte off its element: INVALID_ARG from every entry that checks it, as an
    input and as an output, before anything is launched."""
    torch, L, E, n = torch_cuda, m.load_library(), m.ERR_INVALID_ARG, 256
    a = torch.zeros(n * 8 + 16, dtype=torch.uint8, device="cuda").data_ptr()     # aligned input, and its bad twin
    b = torch.zeros(n * 64 + 16, dtype=torch.uint8, device="cuda").data_ptr()    # aligned outputs
    c = torch.zeros(n * 64 + 16, dtype=torch.uint8, device="cuda").data_ptr()
    prod, blocks, s = ctypes.c_size_t(), ctypes.c_size_t(), _sh(m)
    pb, bb = ctypes.byref(prod), ctypes.byref(blocks)
    d = m.SoftDemapper(m.QAM(4, 0.0, 1.0))
    assert L.modem_demap_process(d._h, a + 1, n, 1.0, b, n * 4, s) == E
    assert L.modem_demap_process(d._h, a, n, 1.0, b + 1, n * 4, s) == E
    d = m.DMPSK(2, 1.0, 0.0, float(np.pi / 2)).detector()
    assert L.modem_diff_process(d._h, a + 1, n, 1.0, b, c, n, s) == E
    assert L.modem_diff_process(d._h, a, n, 1.0, b, c + 1, n, s) == E
    d = m.ToneDetector(np.array([-0.2, 0.2], np.float32), 8)
    assert L.modem_fsk_process(d._h, a + 1, n, 1.0, b, c, None, n, pb, s) == E
    assert L.modem_fsk_process(d._h, a, n, 1.0, b, c + 1, None, n, pb, s) == E
    assert L.modem_fsk_process(d._h, a, n, 1.0, b, None, c + 1, n, pb, s) == E
    d = m.Channel()
    assert L.modem_chan_process(d._h, a + 1, n, b, n, s) == E
    assert L.modem_chan_process(d._h, a, n, b + 1, n, s) == E
    d = m.CarrierSync(4, block=64)
    assert L.modem_sync_process(d._h, a + 1, n, b, n, None, None, 0, pb, bb, s) == E
    assert L.modem_sync_process(d._h, a, n, b + 1, n, None, None, 0, pb, bb, s) == E
    assert L.modem_sync_process(d._h, a, n, b, n, c + 1, None, n, pb, bb, s) == E
    assert L.modem_sync_process(d._h, a, n, b, n, None, c + 1, n, pb, bb, s) == E
    assert d.symbol == 0
    d = m.TimingSync(4, block=64)
    assert L.modem_timing_process(d._h, a + 1, n, b, n, None, None, 0, pb, bb, s) == E
    assert L.modem_timing_process(d._h, a, n, b + 1, n, None, None, 0, pb, bb, s) == E
    assert L.modem_timing_process(d._h, a, n, b, n, c + 1, None, n, pb, bb, s) == E
    assert L.modem_timing_process(d._h, a, n, b, n, None, c + 1, n, pb, bb, s) == E
    assert d.sample == 0
    _, u = _frame_stream()
    d = m.FrameSync(u, guard=FRAME_L, threshold=0.9)
    pos, phi, met, cnt = b, b + 8 * n, b + 16 * n, b + 24 * n
    assert L.modem_frame_process(d._h, a + 1, n, pos, phi, met, n, cnt, s) == E
    assert L.modem_frame_process(d._h, a, n, pos + 1, phi, met, n, cnt, s) == E
    assert L.modem_frame_process(d._h, a, n, pos, phi + 1, met, n, cnt, s) == E
    assert L.modem_frame_process(d._h, a, n, pos, phi, met, n, cnt + 1, s) == E
    assert d.symbol == 0
    f32 = m.DTYPE_F32
    assert L.modem_frame_gather(a + 1, n, 0, pos, phi, cnt, 4, 0, 4, 1, f32, f32, c, c + 8 * n, 0, s) == E
    assert L.modem_frame_gather(a, n, 0, pos + 1, phi, cnt, 4, 0, 4, 1, f32, f32, c, c + 8 * n, 0, s) == E
    assert L.modem_frame_gather(a, n, 0, pos, phi, cnt, 4, 0, 4, 1, f32, f32, c + 1, c + 8 * n, 0, s) == E
    torch.cuda.synchronize()


def test_tx_takes_a_misaligned_device_pointer(m, torch_cuda):
    """TX refuses no alignment: bits at an odd address (4 bits per symbol: not the word loads of the
    aligned case) give the samples of the aligned call."""
    torch = torch_cuda
    bits = np.random.RandomState(10).randint(0, 2, 2004).astype(np.uint8)
    buf = torch.zeros(len(bits) + 1, dtype=torch.uint8, device="cuda")
    view = buf[1:]
    view.copy_(torch.from_numpy(bits))
    assert view.data_ptr() % 2 == 1
    outs = []
    for b in (torch.from_numpy(bits).cuda(), view):
        tx = m.DigitalModulator(m.Carrier(m.Freq(1, 4)), m.QAM(4, 0.0, 1.0), 4, m.rrc_taps(33, 4, 0.35))
        outs.append(_bytes(tx.process(b)))
    assert len(outs[0]) == 2004 * 8 and outs[0] == outs[1]
