"""The convolutional code on the device against the restatement of tests/fec_ref.py, bit for bit:
the encoder, the Viterbi decoder on uniform random LLRs (dense in near-ties), partial waves, every
constraint length, the open trellis, the ok flags, float input through the quantiser, the length
limits and the refusals that need a handle."""
import numpy as np
import pytest

import fec_ref

pytestmark = pytest.mark.gpu

CODES = {(3, 2): (7, 5), (3, 3): (7, 5, 3), (7, 2): (0o171, 0o133), (7, 3): (0o171, 0o133, 0o165),
         (9, 2): (0o753, 0o561), (9, 3): (0o557, 0o663, 0o711)}
MORE = {4: (0o15, 0o17), 5: (0o23, 0o35), 6: (0o53, 0o75), 8: (0o371, 0o247)}
NFRAMES = (1, 17, 130)
NBITS = (1, 63, 64, 65, 442)
SENT = 0xA5


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _encode_raw(m, torch, code, bits, nbits, pad):
    """bits (nframes, in_stride) through the C ABI into rows of n T + pad sentinel bytes."""
    nframes, in_stride = bits.shape
    ncoded = code.coded_bits(nbits)
    b = _dev(torch, bits)
    out = torch.full((nframes, ncoded + pad), SENT, dtype=torch.uint8, device="cuda")
    st = m.load_library().modem_conv_encode(code.K, code._polys(), code.n, code.flags, b.data_ptr(), nframes, nbits, in_stride,
                                            out.data_ptr(), ncoded + pad, 0, m._stream_handle(None, 0))
    assert st == m.MODEM_OK
    o = out.cpu().numpy()
    assert (o[:, ncoded:] == SENT).all()
    return o[:, :ncoded]


def _decode_raw(m, torch, dec, llr, nbits, qscale=1.0, ok=None, pad=3, expect=None):
    """llr (nframes, stride) of the handle's dtype through the C ABI; rows of nbits + pad sentinel bytes."""
    nframes, stride = llr.shape
    x = _dev(torch, llr)
    out = torch.full((nframes, nbits + pad), SENT, dtype=torch.uint8, device="cuda")
    met = torch.full((nframes,), -7, dtype=torch.int32, device="cuda")
    okt = None if ok is None else _dev(torch, ok)
    st = m.load_library().modem_viterbi_process(dec._h, x.data_ptr(), stride, nframes, nbits, qscale,
                                                None if okt is None else okt.data_ptr(), out.data_ptr(), nbits + pad,
                                                met.data_ptr(), m._stream_handle(None, 0))
    o, mt = out.cpu().numpy(), met.cpu().numpy()
    if expect is not None:
        assert st == expect and (o == SENT).all() and (mt == -7).all()
        return None
    assert st == m.MODEM_OK
    assert (o[:, nbits:] == SENT).all()
    return o[:, :nbits], mt


def _check(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what


@pytest.mark.parametrize("K,n", list(CODES))
def test_encoder_equals_the_reference(m, torch_cuda, K, n):
    """Input strides larger than the rows, bytes with high bits set, sentinels past n T intact."""
    rng = np.random.RandomState(100 * K + n)
    code = m.ConvCode(K, CODES[K, n])
    for nframes in NFRAMES:
        for nbits in NBITS:
            bits = rng.randint(0, 256, (nframes, nbits + 3)).astype(np.uint8)
            got = _encode_raw(m, torch_cuda, code, bits, nbits, pad=5)
            assert np.array_equal(got, fec_ref.encode(bits[:, :nbits], K, CODES[K, n])), (nframes, nbits)


@pytest.mark.parametrize("K,n", list(CODES))
def test_decoder_equals_the_reference_on_random_llrs(m, torch_cuda, K, n):
    """Uniform int8, -128 included; the llr stride is larger than n T with garbage in the padding."""
    rng = np.random.RandomState(200 * K + n)
    polys = CODES[K, n]
    dec = m.ConvCode(K, polys).decoder()
    for nframes in NFRAMES:
        for nbits in NBITS:
            llr = rng.randint(-128, 128, (nframes, n * fec_ref.steps(K, nbits) + 5)).astype(np.int8)
            got = _decode_raw(m, torch_cuda, dec, llr, nbits)
            _check(got, fec_ref.decode(fec_ref.quantise(llr), nbits, K, polys), (nframes, nbits))


@pytest.mark.parametrize("K,nframes", [(3, 1), (3, 15), (3, 16), (3, 17), (5, 5)])
def test_partial_last_wave(m, torch_cuda, K, nframes):
    """K = 3 packs 16 frames into a wave, K = 5 four: frame counts around and inside a wave."""
    polys = CODES[3, 2] if K == 3 else MORE[K]
    rng = np.random.RandomState(nframes)
    llr = rng.randint(-128, 128, (nframes, 2 * fec_ref.steps(K, 100))).astype(np.int8)
    got = _decode_raw(m, torch_cuda, m.ConvCode(K, polys).decoder(), llr, 100)
    _check(got, fec_ref.decode(fec_ref.quantise(llr), 100, K, polys), (K, nframes))


@pytest.mark.parametrize("K", sorted(MORE))
def test_every_other_constraint_length(m, torch_cuda, K):
    """K = 4, 5, 6 (8, 4, 2 frames per wave) and K = 8 (two states per lane), tail on and off."""
    rng = np.random.RandomState(K)
    for tail in (True, False):
        code = m.ConvCode(K, MORE[K], tail=tail)
        bits = rng.randint(0, 2, (9, 70)).astype(np.uint8)
        assert np.array_equal(_encode_raw(m, torch_cuda, code, bits, 70, pad=1), fec_ref.encode(bits, K, MORE[K], tail))
        llr = rng.randint(-128, 128, (9, code.coded_bits(70) + 1)).astype(np.int8)
        got = _decode_raw(m, torch_cuda, code.decoder(), llr, 70)
        _check(got, fec_ref.decode(fec_ref.quantise(llr), 70, K, MORE[K], tail), (K, tail))


@pytest.mark.parametrize("K,n", list(CODES))
def test_open_trellis(m, torch_cuda, K, n):
    """TAIL off: the end state is the largest final metric, the lowest index among equals (small
    LLRs make equal final metrics common)."""
    rng = np.random.RandomState(300 * K + n)
    polys = CODES[K, n]
    code = m.ConvCode(K, polys, tail=False)
    dec = code.decoder()
    for nbits, lim in ((1, 128), (65, 128), (442, 128), (40, 2)):
        llr = rng.randint(-lim, lim, (19, n * nbits + 2)).astype(np.int8)
        _check(_decode_raw(m, torch_cuda, dec, llr, nbits), fec_ref.decode(fec_ref.quantise(llr), nbits, K, polys, False), nbits)


def test_all_zero_llrs_decode_to_zeros(m, torch_cuda):
    for (K, n), polys in CODES.items():
        for tail in (True, False):
            code = m.ConvCode(K, polys, tail=tail)
            bits, met = _decode_raw(m, torch_cuda, code.decoder(), np.zeros((5, code.coded_bits(50)), np.int8), 50)
            assert not bits.any() and not met.any()


def test_ok_flags_skip_rows(m, torch_cuda):
    """Mixed 0 / 1 rows, whole waves of zeros included: zeros and metric 0 where ok = 0, the others unchanged."""
    rng = np.random.RandomState(8)
    for (K, n), polys in CODES.items():
        dec = m.ConvCode(K, polys).decoder()
        llr = rng.randint(-128, 128, (70, n * fec_ref.steps(K, 90) + 1)).astype(np.int8)
        ok = rng.randint(0, 2, 70).astype(np.uint8) * rng.choice([1, 2, 255], 70).astype(np.uint8)
        ok[32:48] = 0
        ok[0], ok[1] = 0, 1
        want_bits, want_met = fec_ref.decode(fec_ref.quantise(llr), 90, K, polys)
        want_bits[ok == 0], want_met[ok == 0] = 0, 0
        _check(_decode_raw(m, torch_cuda, dec, llr, 90, ok=ok), (want_bits, want_met), (K, n))


def test_ok_flags_from_the_frame_gather(m, torch_cuda):
    """A short synthetic stream: two unique words, the second too close to the end for its payload,
    cap 4: ok = [1, 0, 0, 0] as FrameSync.gather writes it goes straight into the decoder, with the
    demapper's flat int8 output over frames.view(-1, 2)."""
    torch = torch_cuda
    rng = np.random.RandomState(12)
    qpsk, code, nbits = m.QPSK(0.0, 1.0), m.ConvCode(), 58
    nsym = code.coded_bits(nbits) // 2                                  # 64 payload symbols
    lut = qpsk.lut()
    uw = rng.randint(0, 4, 16)
    x = (lut[rng.randint(0, 4, 400)] + 0.2 * rng.standard_normal((400, 2))).astype(np.float32)
    x[50:66], x[350:366] = lut[uw], lut[uw]
    fs = qpsk.framer(uw, threshold=0.8)
    xs = _dev(torch, x)
    a, b = fs.process(xs, cap=4), fs.flush(like=xs, cap=4)
    ca, cb = int(a[3][0]), int(b[3][0])
    assert ca + cb == 2                                                 # the hits of the call and of the flush, in one list of cap 4
    pos = torch.cat([a[0][:ca], b[0][:cb], torch.zeros(2, dtype=torch.int64, device="cuda")])
    phi = torch.cat([a[1][:ca], b[1][:cb], torch.zeros(2, dtype=torch.int32, device="cuda")])
    cnt = torch.full((1,), 2, dtype=torch.int64, device="cuda")
    assert pos[:2].tolist() == [50, 350]
    frames, ok = fs.gather(xs, 0, pos, phi, cnt, length=nsym)
    assert ok.tolist() == [1, 0, 0, 0]
    llr = qpsk.demapper(out_dtype=m.DTYPE_I8).process(frames.view(-1, 2), scale=8.0)
    bits, met = code.decoder().process(llr, nbits, ok=ok)              # (4 * 64, 2): frames back to back
    same, _ = code.decoder().process(llr, nbits, stride=2 * nsym, ok=ok)
    assert torch.equal(bits, same)
    q = fec_ref.quantise(llr.cpu().numpy().reshape(4, 2 * nsym))
    want_bits, want_met = fec_ref.decode(q, nbits, 7, code.polys)
    want_bits[1:], want_met[1:] = 0, 0
    assert want_met[0] != 0
    _check((bits.cpu().numpy(), met.cpu().numpy()), (want_bits, want_met), "gather")
    both, _ = code.decoder().process(llr.view(4, -1), nbits, want_metric=False)     # 2-D, no flags: every row decoded
    assert np.array_equal(both.cpu().numpy(), fec_ref.decode(q, nbits, 7, code.polys)[0])


@pytest.mark.parametrize("qscale", [1.0, 0.37, 8.0])
@pytest.mark.parametrize("half", [False, True])
def test_float_input_goes_through_the_stated_quantiser(m, torch_cuda, qscale, half):
    """Values at and past +-127 / qscale, exact .5 products (ties to even), infinities, tiny values."""
    rng = np.random.RandomState(int(qscale * 100) + half)
    K, polys, nbits, nframes = 7, CODES[7, 2], 120, 21
    ncol = 2 * fec_ref.steps(K, nbits) + 3
    ft = np.float16 if half else np.float32
    v = rng.uniform(-140, 140, (nframes, ncol)) / qscale
    pick = rng.randint(0, 8, v.shape)
    halves = (rng.randint(-130, 130, v.shape) + 0.5) / qscale
    edge = rng.choice([127.0, -127.0, 127.5, -127.5, 126.5, -126.5, 128.0, -128.0], v.shape) / qscale
    v = np.where(pick == 0, halves, np.where(pick == 1, edge, np.where(pick == 2, rng.choice([np.inf, -np.inf, 1e-30, 0.0, -0.0], v.shape), v)))
    v = v.astype(ft)
    if not half:                                                        # f32: the nearest values on either side of the edges too
        v[0, :8] = np.nextafter(np.float32(127.5 / qscale), np.float32([np.inf, -np.inf] * 4))
    q = fec_ref.quantise(v, qscale)
    if qscale != 0.37:
        fin = v[np.isfinite(v)].astype(np.float64)
        assert np.mean(np.abs(fin * qscale % 1.0) == 0.5) > 0.05                       # exact ties are in the input
    assert (np.abs(q) == 127).mean() > 0.05
    dec = m.ConvCode(K, polys).decoder(in_dtype=m.DTYPE_F16 if half else m.DTYPE_F32)
    _check(_decode_raw(m, torch_cuda, dec, v, nbits, qscale=qscale), fec_ref.decode(q, nbits, K, polys), (qscale, half))


@pytest.mark.parametrize("K,n", [(7, 2), (7, 3), (9, 2), (8, 2)])
def test_at_and_over_the_length_limit(m, torch_cuda, K, n):
    """One frame with T exactly at the limit; one step over is INVALID_ARG and nothing is written."""
    polys = CODES[K, n] if (K, n) in CODES else MORE[K]
    T = fec_ref.MAX_STEPS[K]
    nbits = T - (K - 1)
    rng = np.random.RandomState(K)
    dec = m.ConvCode(K, polys).decoder()
    llr = rng.randint(-128, 128, (1, n * (T + 1))).astype(np.int8)
    _check(_decode_raw(m, torch_cuda, dec, llr, nbits), fec_ref.decode(fec_ref.quantise(llr), nbits, K, polys), K)
    _decode_raw(m, torch_cuda, dec, llr, nbits + 1, expect=m.ERR_INVALID_ARG)
    open_dec = m.ConvCode(K, polys, tail=False).decoder()
    _check(_decode_raw(m, torch_cuda, open_dec, llr, T), fec_ref.decode(fec_ref.quantise(llr), T, K, polys, False), K)
    _decode_raw(m, torch_cuda, open_dec, llr, T + 1, expect=m.ERR_INVALID_ARG)


def test_noiseless_round_trip_through_the_encoder(m, torch_cuda):
    torch = torch_cuda
    for (K, n), polys in CODES.items():
        for tail in (True, False):
            code = m.ConvCode(K, polys, tail=tail)
            bits = m.prng_bits(K * 8 + n, 33 * 442).view(33, 442)
            coded = code.encode(bits)
            assert tuple(coded.shape) == (33, code.coded_bits(442))
            llr = (100 - 200 * coded.to(torch.int16)).to(torch.int8)
            got, met = code.decoder().process(llr, 442)
            assert torch.equal(got, bits) and bool((met == 100 * code.coded_bits(442)).all())


def test_process_refusals(m, torch_cuda):
    """The refusals that need a handle: nothing is written. Host memory is refused too."""
    K, polys, nbits = 7, CODES[7, 2], 30
    ncoded = 2 * fec_ref.steps(K, nbits)
    llr = np.ones((3, ncoded), np.int8)
    dec = m.ConvCode(K, polys).decoder()
    t = torch_cuda
    for qs in (0.0, -1.0, float("inf"), float("nan")):
        _decode_raw(m, t, dec, llr, nbits, qscale=qs, expect=m.ERR_INVALID_ARG)
    _decode_raw(m, t, dec, llr, 0, expect=m.ERR_INVALID_ARG)
    _decode_raw(m, t, dec, llr, nbits + 1, expect=m.ERR_INVALID_ARG)             # stride < n T
    _decode_raw(m, t, dec, llr, nbits, pad=-1, expect=m.ERR_INVALID_ARG)         # out_stride < nbits
    L = m.load_library()
    x, out = _dev(t, llr), t.full((3, nbits), SENT, dtype=t.uint8, device="cuda")
    host = np.zeros((3, ncoded), np.int8)
    args = lambda a, o: (dec._h, a, ncoded, 3, nbits, 1.0, None, o, nbits, None, m._stream_handle(None, 0))
    assert L.modem_viterbi_process(*args(None, out.data_ptr())) == m.ERR_INVALID_ARG
    assert L.modem_viterbi_process(*args(x.data_ptr(), None)) == m.ERR_INVALID_ARG
    assert L.modem_viterbi_process(*args(host.ctypes.data, out.data_ptr())) == m.ERR_INVALID_ARG
    assert L.modem_viterbi_process(dec._h, None, ncoded, 0, nbits, 1.0, None, None, nbits, None, None) == m.MODEM_OK
    f32 = m.ConvCode(K, polys).decoder(in_dtype=m.DTYPE_F32)
    xf = t.zeros(3 * ncoded + 1, dtype=t.float16, device="cuda")
    assert L.modem_viterbi_process(f32._h, xf.data_ptr() + 2, ncoded, 1, nbits, 1.0, None, out.data_ptr(), nbits, None,
                                   None) == m.ERR_INVALID_ARG                    # an f32 buffer must be 4-byte aligned
    assert bool((out == SENT).all())
    code = m.ConvCode(K, polys)
    bits = t.zeros((2, 10), dtype=t.uint8, device="cuda")
    enc = lambda nframes, b, o: L.modem_conv_encode(K, code._polys(), 2, 1, b, nframes, 10, 10, o, 32, 0, None)
    assert enc(0, None, None) == m.MODEM_OK
    assert enc(2, np.zeros((2, 10), np.uint8).ctypes.data, out.data_ptr()) == m.ERR_INVALID_ARG
    assert enc(2, bits.data_ptr(), out.data_ptr()) == m.MODEM_OK
    with pytest.raises(m.ModemPanic):                                            # one step over the limit, through Python
        dec.process(t.zeros((1, 2 * 4097), dtype=t.int8, device="cuda"), 4091)
    with pytest.raises(ValueError):                                              # 216 values are not whole frames of 8192
        dec.process(x, 4090)
