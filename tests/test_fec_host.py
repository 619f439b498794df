"""Convolutional code, host side (no device needed): the restatement of tests/fec_ref.py is a
maximum-likelihood decoder (checked exhaustively on a small code) and meets the tie and round-trip
rules; the host decoder of tests/cpp/fec_host.cpp, which compiles the product's own
modem_fec_math.h, equals it bit for bit under the address and undefined-behaviour sanitizers; the
C ABI entry points exist and refuse bad arguments before they look for a device; and the
restatement alone, behind the oracle's loopback, meets the condition that
tests/test_gpu_fec_loopback.py puts on the device."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import chan_ref
import fec_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_DEVICE = 1 << 20
SYMBOLS = ("modem_conv_encode", "modem_viterbi_create", "modem_viterbi_process", "modem_viterbi_destroy")
CODES = [(3, (7, 5)), (3, (7, 5, 3)), (7, (0o171, 0o133)), (7, (0o171, 0o133, 0o165)), (9, (0o753, 0o561)),
         (9, (0o557, 0o663, 0o711))]


# ----------------------------------------------------------------- the restatement ----
def test_reference_is_maximum_likelihood_exhaustively():
    """K = 3 (7, 5), 8 information bits: over 200 random integer LLR rows the metric is the largest
    correlation over all 256 codewords, and the decoded word re-encoded has that correlation."""
    K, polys, nbits = 3, (7, 5), 8
    words = ((np.arange(256)[:, None] >> np.arange(nbits)[::-1]) & 1).astype(np.uint8)
    code = fec_ref.encode(words, K, polys)
    assert code.shape == (256, fec_ref.coded_bits(K, 2, nbits)) and len({c.tobytes() for c in code}) == 256
    rng = np.random.RandomState(3)
    q = rng.randint(-127, 128, (200, code.shape[1]))
    best = fec_ref.correlation(code, q).max(1)
    bits, metric = fec_ref.decode(q, nbits, K, polys)
    assert np.array_equal(metric, best)
    again = fec_ref.encode(bits, K, polys)
    assert np.array_equal(np.sum((1 - 2 * again.astype(np.int64)) * q, 1), best)


def test_all_zero_llrs_give_all_zero_bits():
    """Every metric ties at 0 and ties keep predecessor 0: the all-zero path, with and without the tail."""
    for K, polys in CODES:
        for tail in (True, False):
            bits, metric = fec_ref.decode(np.zeros((3, 3 * (40 + K))), 40, K, polys, tail)
            assert not bits.any() and not metric.any()


@pytest.mark.parametrize("K,polys", CODES)
@pytest.mark.parametrize("tail", [True, False])
def test_noiseless_round_trip_is_the_identity(K, polys, tail):
    rng = np.random.RandomState(K * 10 + len(polys))
    bits = rng.randint(0, 2, (9, 77)).astype(np.uint8)
    code = fec_ref.encode(bits | 0xF0, K, polys, tail)                  # only bit 0 of a byte counts
    assert code.shape[1] == fec_ref.coded_bits(K, len(polys), 77, tail) and code.max() <= 1
    got, metric = fec_ref.decode(100 * (1 - 2 * code.astype(np.int64)), 77, K, polys, tail)
    assert np.array_equal(got, bits)                                    # open trellis too: the sent path alone reaches 100 n T
    assert (metric == 100 * code.shape[1]).all()


def test_quantiser_rule():
    assert fec_ref.quantise(np.array([-128, -127, 0, 127], np.int8)).tolist() == [-127, -127, 0, 127]
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 126.5, 127.5, 1e9, -1e9, 0.49999997], np.float32)
    assert fec_ref.quantise(v, 1.0).tolist() == [0, 2, 2, 0, -2, 126, 127, 127, -127, 0]
    assert fec_ref.quantise(np.array([1.0, 3.0, -5.0], np.float16), 0.5).tolist() == [0, 2, -2]


# ------------------------------------------------------------- the host C++ decoder ----
@pytest.fixture(scope="module")
def fec_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fec_host") / "fec_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "rust-modem_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "fec_host.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("K,polys", CODES)
def test_host_decoder_equals_the_reference(fec_host, tmp_path, K, polys):
    """Uniform random int8 LLRs, -128 included (dense in near-ties), padding between the rows."""
    rng = np.random.RandomState(K + len(polys))
    n = len(polys)
    for tail, nbits, nframes in ((True, 1, 3), (True, 65, 7), (False, 64, 5), (True, 442, 4)):
        T = fec_ref.steps(K, nbits, tail)
        stride = n * T + 5
        llr = rng.randint(-128, 128, (nframes, stride)).astype(np.int8)
        fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
        llr.tofile(fin)
        subprocess.run([fec_host, str(K), str(int(tail)), str(nbits), str(nframes), str(stride), str(fin), str(fout),
                        *[str(g) for g in polys]], check=True, stdout=subprocess.DEVNULL)
        raw = np.fromfile(fout, np.uint8)
        assert raw.size == nframes * nbits + 4 * nframes
        bits, metric = fec_ref.decode(fec_ref.quantise(llr), nbits, K, polys, tail)
        assert np.array_equal(raw[:nframes * nbits].reshape(nframes, nbits), bits)
        assert np.array_equal(raw[nframes * nbits:].view(np.int32), metric)


# ------------------------------------------------------------------------ the C ABI ----
def _polys(p):
    return (ctypes.c_uint32 * len(p))(*p)


def _create(m, K=7, polys=(0o171, 0o133), n=None, flags=1, in_dtype=None, device=0, out="handle", null_polys=False):
    h = ctypes.c_void_p(0xDEAD)
    st = m.load_library().modem_viterbi_create(K, None if null_polys else _polys(polys), len(polys) if n is None else n, flags,
                                               m.DTYPE_I8 if in_dtype is None else in_dtype, device,
                                               None if out is None else ctypes.byref(h))
    return st, h


BAD_CODES = [dict(K=2), dict(K=10), dict(K=0), dict(n=1), dict(n=4), dict(n=0), dict(polys=(0, 0o133)), dict(polys=(0o171, 128)),
             dict(polys=(0o171, 0o133, 1 << 31)), dict(K=3, polys=(7, 8)), dict(flags=2), dict(flags=3), dict(null_polys=True)]


def test_library_exports_the_convolutional_code(m):
    lib = ctypes.CDLL(m.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert m.load_library().modem_abi_version() == 6      # additive: the version stays
    for name in ("ConvCode", "ViterbiDecoder", "CONV_TAIL"):
        assert name in m.__all__ and hasattr(m, name)
    code = m.ConvCode()
    assert (code.K, code.polys, code.tail) == (7, (0o171, 0o133), True)
    assert code.coded_bits(442) == 896 == fec_ref.coded_bits(7, 2, 442)
    assert m.ConvCode(9, (0o557, 0o663, 0o711), tail=False).coded_bits(10) == 30


@pytest.mark.parametrize("device", [0, BAD_DEVICE])
def test_create_refusals_come_before_the_device(m, device):
    for kw in BAD_CODES + [dict(in_dtype=m.DTYPE_I16), dict(in_dtype=-1), dict(in_dtype=4)]:
        st, h = _create(m, device=device, **kw)
        assert st == m.ERR_INVALID_ARG, kw
        assert h.value is None, kw
    st, _ = _create(m, device=device, out=None)
    assert st == m.ERR_INVALID_ARG
    for kw in (dict(K=2), dict(K=10), dict(polys=(0o171,)), dict(polys=(0o171, 0o133, 0o165, 1)), dict(polys=(0, 1))):
        with pytest.raises(m.ModemPanic):
            m.ConvCode(**{"K": 7, "polys": (0o171, 0o133), **kw})
    with pytest.raises(m.ModemPanic):
        m.ConvCode().decoder(in_dtype=m.DTYPE_I16, device=device)


def test_a_bad_ordinal_is_no_device(m):
    for device in (BAD_DEVICE, -1):
        for K, polys in CODES:
            st, h = _create(m, K=K, polys=polys, device=device)
            assert st == m.ERR_NO_DEVICE and h.value is None
    assert m.load_library().modem_viterbi_destroy(None) == m.MODEM_OK


@pytest.mark.parametrize("device", [0, BAD_DEVICE])
def test_encode_refusals_come_before_the_device(m, device):
    L = m.load_library()
    bits, out = np.zeros((2, 16), np.uint8), np.zeros((2, 64), np.uint8)
    a = lambda v: None if v is None else v.ctypes.data

    def enc(K=7, polys=(0o171, 0o133), n=None, flags=1, bits_=bits, nframes=2, nbits=10, in_stride=16, out_=out, out_stride=64,
            null_polys=False):
        return L.modem_conv_encode(K, None if null_polys else _polys(polys), len(polys) if n is None else n, flags, a(bits_),
                                   nframes, nbits, in_stride, a(out_), out_stride, device, None)
    for kw in BAD_CODES + [dict(nbits=0), dict(in_stride=9), dict(out_stride=31), dict(flags=0, out_stride=19), dict(bits_=None),
                           dict(out_=None), dict(nbits=1 << 62, in_stride=1 << 62, out_stride=1 << 63)]:
        assert enc(**kw) == m.ERR_INVALID_ARG, kw
    assert enc(out_stride=32) != m.ERR_INVALID_ARG                     # n * T = 2 * 16 fits exactly
    assert enc(flags=0, out_stride=20) != m.ERR_INVALID_ARG
    if device == BAD_DEVICE:
        assert enc() == m.ERR_NO_DEVICE and enc(nframes=0, bits_=None, out_=None) == m.ERR_NO_DEVICE


def test_process_refuses_a_null_handle(m):
    L = m.load_library()
    x = np.zeros(64, np.uint8)
    assert L.modem_viterbi_process(None, x.ctypes.data, 32, 1, 10, 1.0, None, x.ctypes.data, 10, None, None) == m.ERR_INVALID_ARG


# ------------------------------------------------- the loopback condition, on the CPU ----
LOOP = dict(K=7, polys=(0o171, 0o133), nframes=256, nbits=442, ebn0_db=3.0, qs=8.0, seed=0xFEC0, noise_seed=77, sps=4, L=65)


def loop_n0():
    """QPSK of amplitude 1 (2 coded bits per symbol), rate 1/2: n0 = A^2 / (bps R Eb/N0)."""
    return 1.0 / (2 * 0.5 * 10.0 ** (LOOP["ebn0_db"] / 10))


def loop_limit():
    """A tenth of the uncoded expectation at the same information Eb/N0 (2589.9 of 113152), rounded."""
    nbits = LOOP["nframes"] * LOOP["nbits"]
    return round(nbits * 0.5 * math.erfc(math.sqrt(10.0 ** (LOOP["ebn0_db"] / 10))) / 10)


def demap_i8(r, lut, scale):
    """The demapper's rule in numpy: llr_j = scale (min_{bit_j = 1} |r - s|^2 - min_{bit_j = 0} |r - s|^2),
    j = 0 the MSB, as int8 = rint(clamp(llr, -127, 127))."""
    bps = int(lut.shape[0]).bit_length() - 1
    z = r[:, 0].astype(np.float64) + 1j * r[:, 1].astype(np.float64)
    pts = lut[:, 0].astype(np.float64) + 1j * lut[:, 1].astype(np.float64)
    d = np.abs(z[:, None] - pts[None, :]) ** 2
    idx = np.arange(lut.shape[0])
    llr = np.stack([d[:, (idx >> (bps - 1 - j)) & 1 == 1].min(1) - d[:, (idx >> (bps - 1 - j)) & 1 == 0].min(1) for j in range(bps)], 1)
    return np.rint(np.clip(scale * llr, -127, 127)).astype(np.int8)


def test_reference_meets_the_loopback_condition(m, o):
    """The oracle's TX and RX around chan_ref.channel, the numpy demapper quantised to int8 with
    qs = 8, fec_ref's decoder: at an information Eb/N0 of 3 dB the decoded bit errors are at most a
    tenth of what uncoded QPSK would make (2590 expected of 113152, so at most 259)."""
    C = LOOP
    assert loop_limit() == 259
    K, polys, nframes, nbits = C["K"], C["polys"], C["nframes"], C["nbits"]
    sps, L = C["sps"], C["L"]
    n0 = loop_n0()
    bits = o.prng_bits(C["seed"], nframes * nbits).reshape(nframes, nbits)
    coded = fec_ref.encode(bits, K, polys)
    taps = m.rrc_taps(L, sps, 0.35)
    w = o.sample_freq(1, 4)
    x = o.tx_chain(o.new_phasor(o.QPSK, 0.0, 1.0), coded.reshape(-1), sps, taps, w, 0, flush_syms=(L - 1 + sps - 1) // sps)
    y, _ = chan_ref.channel(x, n0=n0, seed=C["noise_seed"])
    riq, _ = o.rx_chain(y.astype(np.float32), w, 0, o.MIX_COMPLEX, taps, sps, L - 1, None)
    lut = o.phasor_lut(o.new_phasor(o.QPSK, 0.0, 1.0))
    nsym = coded.size // 2
    llr = demap_i8(riq[:nsym], lut, C["qs"] / n0).reshape(nframes, -1)
    raw = int(np.sum((llr < 0) != (coded == 1)))
    got, _ = fec_ref.decode(fec_ref.quantise(llr), nbits, K, polys)
    errors = int(np.sum(got != bits))
    print(f"reference coded loopback at {C['ebn0_db']} dB: {errors} decoded bit errors of {bits.size} (limit {loop_limit()}), "
          f"{raw} raw errors of {coded.size} coded bits")
    assert errors <= loop_limit()
