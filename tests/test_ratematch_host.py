"""Rate matching and the frame check, host side (no device needed): the restatement of
tests/ratematch_ref.py meets the facts of include/modem_hip.h, "Rate matching and frame check" (the
interleaver is a bijection, rx undoes tx, the published CRC check values, a single flipped bit is
seen); the host program of tests/cpp/ratematch_host.cpp, which compiles the product's own
modem_ratematch_math.h and folds 64 chunk registers as the kernel does, equals it under the address
and undefined-behaviour sanitizers; the C ABI entry points exist and refuse bad arguments before
they look for a device; and the restatement alone, behind the oracle's loopback, meets the
conditions that tests/test_gpu_ratematch_loopback.py puts on the device."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import chan_ref
import fec_ref
import ratematch_ref as R
from test_fec_host import demap_i8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_DEVICE = 1 << 20
SYMBOLS = ("modem_rm_kept", "modem_rm_tx", "modem_rm_rx", "modem_crc_attach", "modem_crc_check")
P64 = tuple(1 if i == 37 else 0 for i in range(64))
PATTERNS = [(1,), R.PUNCTURE_2_3, R.PUNCTURE_3_4, P64, (0, 1, 1), (1, 0, 0, 0, 1)]
# (W, poly, init, check value of "123456789")
CHECK_VALUES = [(16, 0x1021, 0xFFFF, 0x29B1), (16, 0x1021, 0, 0x31C3), (32, 0x04C11DB7, 0xFFFFFFFF, 0x0376E6E7),
                (8, 0x07, 0, 0xF4), (24, 0x864CFB, 0xB704CE, 0x21CF02)]
# every width with init and xorout nonzero
CRCS = [(8, 0x07, 0x5A, 0xC3), (16, 0x1021, 0xFFFF, 0x1D0F), (24, 0x864CFB, 0xB704CE, 0x00F00F), (32, 0x04C11DB7, 0xFFFFFFFF, 0xDEADBEEF)]


# ----------------------------------------------------------------- the restatement ----
def test_pi_is_a_bijection():
    """C = 1 (the identity), C > E, cl = C (E a multiple of C) and cl = 1 among the grid."""
    seen = set()
    for E in (1, 2, 5, 31, 32, 33, 64, 65, 97, 598, 672, 1025):
        for C in (1, 2, 3, 7, 31, 32, 33, 64, 96, 255, 256):
            rows = -(-E // C)
            cl = E - (rows - 1) * C
            seen.add(("C1" if C == 1 else "C>E" if C > E else "cl=C" if cl == C else "cl=1" if cl == 1 else "other"))
            out = [R.pi(j, E, C) for j in range(E)]
            assert sorted(out) == list(range(E)), (E, C)
            if C == 1:
                assert out == list(range(E))
    assert seen == {"C1", "C>E", "cl=C", "cl=1", "other"}


def test_rank_counts_the_kept_indices_below():
    for pat in PATTERNS:
        ms = [m for m in range(400) if R.is_kept(pat, m)]
        assert [R.rank(pat, m) for m in ms] == list(range(len(ms)))
    assert R.kept(R.PUNCTURE_2_3, 896) == 672 and R.kept(R.PUNCTURE_3_4, 896) == 598


def test_rx_of_tx_restores_the_kept_and_zeros_the_rest():
    rng = np.random.RandomState(1)
    for pat in PATTERNS:
        for C in (1, 7, 32, 255):
            for nm in (64, 65, 897):
                if R.kept(pat, nm) == 0:
                    continue
                x = rng.randint(0, 256, (3, nm)).astype(np.uint8)
                y = R.tx(x, pat, C)
                assert y.shape == (3, R.kept(pat, nm)) and y.max() <= 1
                back = R.rx(y, nm, pat, C)
                keep = np.array([R.is_kept(pat, m) for m in range(nm)])
                assert np.array_equal(back[:, keep], x[:, keep] & 1) and not back[:, ~keep].any()


def _ascii_bits(text):
    return np.array([(ord(ch) >> (7 - i)) & 1 for ch in text for i in range(8)], np.uint8)


@pytest.mark.parametrize("W,poly,init,value", CHECK_VALUES)
def test_crc_check_values(W, poly, init, value):
    msg = _ascii_bits("123456789")
    assert msg.size == 72
    assert R.crc(msg, W, poly, init) == value
    assert int(R.crc_rows(msg[None, :], W, poly, init)[0]) == value


@pytest.mark.parametrize("W,poly,init,xorout", CRCS)
def test_check_of_attach_and_single_bit_flips(W, poly, init, xorout):
    rng = np.random.RandomState(W)
    b = rng.randint(0, 256, (4, 37)).astype(np.uint8)                  # only bit 0 of a byte counts
    a = R.attach(b, W, poly, init, xorout)
    assert a.shape == (4, 37 + W) and a.max() <= 1 and np.array_equal(a[:, :37], b & 1)
    assert R.check(a, W, poly, init, xorout).tolist() == [1, 1, 1, 1]
    assert R.check(a | 0xFE, W, poly, init, xorout).tolist() == [1, 1, 1, 1]
    assert R.check(a, W, poly, init, xorout, ok=np.array([1, 0, 7, 0])).tolist() == [1, 0, 1, 0]
    for pos in range(37 + W):                                           # any single bit of a row
        bad = a.copy()
        bad[2, pos] ^= 1
        assert R.check(bad, W, poly, init, xorout).tolist() == [1, 1, 0, 1], pos


# ---------------------------------------------------------------- the host C++ program ----
@pytest.fixture(scope="module")
def rm_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ratematch_host") / "ratematch_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "rust-modem_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "ratematch_host.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("W,poly,init,xorout", CRCS)
def test_chunked_crc_equals_the_definition(rm_host, tmp_path, W, poly, init, xorout):
    """Rows shorter than the 64 chunks, chunks of unequal length, a whole frame and a long row; bytes with high bits set."""
    rng = np.random.RandomState(W + 1)
    for nbits in (1, 7, 63, 64, 65, 442 + W, 4097):
        stride, nframes = nbits + 3, 5
        rows = rng.randint(0, 256, (nframes, stride)).astype(np.uint8)
        rows[0, :nbits] = 0
        rows[1, :nbits] = 1
        fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
        rows.tofile(fin)
        subprocess.run([rm_host, "crc", str(W), str(poly), str(init), str(xorout), str(nbits), str(nframes), str(stride),
                        str(fin), str(fout)], check=True)
        got = np.fromfile(fout, np.uint32)
        want = R.crc_rows(rows[:, :nbits], W, poly, init, xorout)
        assert np.array_equal(got.astype(np.uint64), want), (W, nbits)
        assert int(want[3]) == R.crc(rows[3, :nbits], W, poly, init, xorout)


@pytest.mark.parametrize("pat", PATTERNS)
def test_host_rank_and_pi_equal_the_restatement(rm_host, tmp_path, pat):
    for C in (1, 7, 32, 255, 256):
        for nm in (1, 5, 63, 64, 65, 896, 897, 16384):
            E = R.kept(pat, nm)
            if E == 0:
                continue
            fout = tmp_path / "out.bin"
            subprocess.run([rm_host, "rm", "".join(str(v) for v in pat), str(C), str(nm), str(fout)], check=True)
            got = np.fromfile(fout, np.uint32)
            assert got.size == 1 + nm and int(got[0]) == E
            ms, pos = R.positions(pat, nm, C)
            want = np.full(nm, 0xFFFFFFFF, np.uint32)
            want[ms] = pos
            assert np.array_equal(got[1:], want), (C, nm)


# ------------------------------------------------------------------------ the C ABI ----
def test_library_exports_rate_matching_and_the_crc(m):
    lib = ctypes.CDLL(m.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert m.load_library().modem_abi_version() == 6      # additive: the version stays
    for name in ("RateMatch", "CRC", "PUNCTURE_2_3", "PUNCTURE_3_4"):
        assert name in m.__all__ and hasattr(m, name)
    assert m.PUNCTURE_2_3 == R.PUNCTURE_2_3 == m.RateMatch.PUNCTURE_2_3
    assert m.PUNCTURE_3_4 == R.PUNCTURE_3_4 == m.RateMatch.PUNCTURE_3_4
    rm = m.ConvCode().rate_match(m.PUNCTURE_3_4, cols=32)
    assert isinstance(rm, m.RateMatch) and (rm.pattern, rm.cols) == (R.PUNCTURE_3_4, 32)
    assert rm.kept(896) == 598 and m.RateMatch(m.PUNCTURE_2_3).kept(896) == 672
    for pat in PATTERNS:
        for nm in (1, 5, 63, 64, 65, 896, 16384):
            if R.kept(pat, nm):
                assert m.RateMatch(pat).kept(nm) == R.kept(pat, nm)
    c = m.CRC.ccitt16()
    assert (c.width, c.poly, c.init, c.xorout) == (16, 0x1021, 0xFFFF, 0)
    c = m.CRC.mpeg32()
    assert (c.width, c.poly, c.init, c.xorout) == (32, 0x04C11DB7, 0xFFFFFFFF, 0)


def test_python_constructors_refuse(m):
    for kw in (dict(pattern=()), dict(pattern=(0, 0)), dict(pattern=(1, 2)), dict(pattern=(1,) * 65), dict(cols=0), dict(cols=257)):
        with pytest.raises(m.ModemPanic):
            m.RateMatch(**{"pattern": (1, 1, 0), "cols": 4, **kw})
    for a in ((12, 1), (16, 1 << 16), (8, 7, 256), (8, 7, 0, 256), (0, 0)):
        with pytest.raises(m.ModemPanic):
            m.CRC(*a)
    with pytest.raises(m.ModemPanic):
        m.RateMatch(P64).kept(37)                                       # E == 0 for this Nm
    with pytest.raises(m.ModemPanic):
        m.RateMatch().kept(16385)


def _pat(p):
    return (ctypes.c_uint8 * len(p))(*p)


@pytest.mark.parametrize("device", [0, BAD_DEVICE])
def test_rate_match_refusals_come_before_the_device(m, device):
    L = m.load_library()
    buf = np.zeros(1 << 16, np.uint8)
    a, b = buf.ctypes.data, buf.ctypes.data + (1 << 15)

    def tx(pattern=(1, 1, 1, 0), P=None, cols=8, in_=a, nframes=2, nm=100, in_stride=100, out=b, out_stride=75, null_pattern=False):
        return L.modem_rm_tx(None if null_pattern else _pat(pattern), len(pattern) if P is None else P, cols, in_, nframes, nm,
                             in_stride, out, out_stride, device, None)

    def rx(pattern=(1, 1, 1, 0), P=None, cols=8, dtype=m.DTYPE_I8, in_=a, nframes=2, nm=100, in_stride=75, out=b, out_stride=100,
           null_pattern=False):
        return L.modem_rm_rx(None if null_pattern else _pat(pattern), len(pattern) if P is None else P, cols, dtype, in_, nframes,
                             nm, in_stride, None, out, out_stride, device, None)
    common = [dict(P=0), dict(pattern=(1,) * 65), dict(pattern=(1, 2, 1, 0)), dict(pattern=(0, 0, 0)), dict(cols=0), dict(cols=257),
              dict(nm=0), dict(nm=16385), dict(pattern=P64, nm=37), dict(null_pattern=True), dict(in_=None), dict(out=None),
              dict(out=a), dict(out=a + 100), dict(in_=b + 10)]
    for kw in common + [dict(in_stride=99), dict(out_stride=74)]:
        assert tx(**kw) == m.ERR_INVALID_ARG, kw
    for kw in common + [dict(in_stride=74), dict(out_stride=99), dict(dtype=m.DTYPE_I16), dict(dtype=-1), dict(dtype=4)]:
        assert rx(**kw) == m.ERR_INVALID_ARG, kw
    if device == BAD_DEVICE:
        assert tx() == m.ERR_NO_DEVICE and rx() == m.ERR_NO_DEVICE and rx(dtype=m.DTYPE_F32, out=a + (1 << 14)) == m.ERR_NO_DEVICE
        assert tx(nframes=0, in_=None, out=None) == m.ERR_NO_DEVICE and rx(nframes=0, in_=None, out=None) == m.ERR_NO_DEVICE
        assert tx(out=a + 200) == m.ERR_NO_DEVICE                      # the ranges end at 200 and touch only
    kept = ctypes.c_size_t(7)
    assert L.modem_rm_kept(_pat((1, 1, 0)), 3, 10, None) == m.ERR_INVALID_ARG
    assert L.modem_rm_kept(None, 3, 10, ctypes.byref(kept)) == m.ERR_INVALID_ARG
    assert L.modem_rm_kept(_pat((1, 1, 0)), 3, 10, ctypes.byref(kept)) == m.MODEM_OK and kept.value == 7


@pytest.mark.parametrize("device", [0, BAD_DEVICE])
def test_crc_refusals_come_before_the_device(m, device):
    L = m.load_library()
    buf = np.zeros(1 << 12, np.uint8)
    a, b = buf.ctypes.data, buf.ctypes.data + (1 << 11)

    def attach(W=16, poly=0x1021, init=0xFFFF, xorout=0, in_=a, nframes=2, nbits=100, in_stride=100, out=b, out_stride=116):
        return L.modem_crc_attach(W, poly, init, xorout, in_, nframes, nbits, in_stride, out, out_stride, device, None)

    def check(W=16, poly=0x1021, init=0xFFFF, xorout=0, in_=a, nframes=2, nbits=100, in_stride=116, ok_in=None, ok_out=b):
        return L.modem_crc_check(W, poly, init, xorout, in_, nframes, nbits, in_stride, ok_in, ok_out, device, None)
    common = [dict(W=0), dict(W=12), dict(W=33), dict(W=64), dict(poly=1 << 16), dict(init=1 << 16), dict(xorout=1 << 16),
              dict(W=8, poly=0x107), dict(nbits=0), dict(nbits=65537, in_stride=1 << 17), dict(in_=None)]
    for kw in common + [dict(in_stride=99), dict(out_stride=115), dict(out=None), dict(out=a), dict(out=a + 199)]:
        assert attach(**kw) == m.ERR_INVALID_ARG, kw
    for kw in common + [dict(in_stride=115), dict(ok_out=None), dict(ok_out=a + 231)]:
        assert check(**kw) == m.ERR_INVALID_ARG, kw
    if device == BAD_DEVICE:
        assert attach() == m.ERR_NO_DEVICE and check() == m.ERR_NO_DEVICE and check(ok_in=b, ok_out=b) == m.ERR_NO_DEVICE
        assert attach(W=32, poly=0x04C11DB7, init=0xFFFFFFFF, xorout=0xFFFFFFFF, out_stride=132) == m.ERR_NO_DEVICE
        assert attach(nframes=0, in_=None, out=None) == m.ERR_NO_DEVICE and check(nframes=0, in_=None, ok_out=None) == m.ERR_NO_DEVICE
        assert attach(nbits=65536, nframes=1, in_stride=65536, out_stride=65552, out=a + (1 << 20)) == m.ERR_NO_DEVICE


# ----------------------------------------------- the LDS reads of rm_rx, by the bank model ----
def test_rm_rx_lds_reads_of_the_measured_case():
    """rm_rx_kernel<uint8_t> reads LDS at byte pi(rank(m)) for the 64 consecutive m of a wave (a
    punctured lane reads nothing). Byte and dword reads bank on (address / 4) mod 32 within each
    32-lane half, equal dwords broadcast. For the case tools/ratematch_rate.py measures (rate 3/4,
    Nm = 928, 32 columns) the kept lanes of a half are 21 or 22 consecutive ranks, so consecutive
    columns, `rows` = 20 bytes = 5 dwords apart: 5 is odd, so up to 32 consecutive columns fall on
    32 different banks, and only where the ranks wrap from column 31 to column 0 can two dwords
    share a bank: at most 2 addresses on a bank, one extra cycle."""
    pat, nm, C = R.PUNCTURE_3_4, 928, 32
    E = R.kept(pat, nm)
    assert E == 619 and -(-E // C) == 20
    ms, pos = R.positions(pat, nm, C)
    where = dict(zip(ms.tolist(), pos.tolist()))
    worst = 0
    for m0 in range(0, nm, 32):
        banks = {}
        for m in range(m0, min(m0 + 32, nm)):
            if m in where:
                banks.setdefault((where[m] // 4) % 32, set()).add(where[m] // 4)
        worst = max(worst, max(len(v) for v in banks.values()))
    assert worst <= 2


# ------------------------------------------------ the loopback conditions, on the CPU ----
LOOP = dict(K=7, polys=(0o171, 0o133), nframes=256, nbits=442, ebn0_db=4.5, qs=8.0, seed=0xC0DE, noise_seed=78, sps=4, L=65,
            pattern=R.PUNCTURE_3_4, cols=32, crc=(16, 0x1021, 0xFFFF, 0))


def loop_rate():
    """R = information bits over transmitted coded bits of a frame: the CRC and the tail are overhead."""
    C = LOOP
    nm = fec_ref.coded_bits(C["K"], 2, C["nbits"] + C["crc"][0])
    return C["nbits"] / R.kept(C["pattern"], nm)


def loop_n0():
    """QPSK of amplitude 1 (2 coded bits per symbol): n0 = 1 / (2 R Eb/N0)."""
    return 1.0 / (2 * loop_rate() * 10.0 ** (LOOP["ebn0_db"] / 10))


def loop_limit():
    """A tenth of the uncoded expectation at the same information Eb/N0, rounded."""
    n = LOOP["nframes"] * LOOP["nbits"]
    return round(n * 0.5 * math.erfc(math.sqrt(10.0 ** (LOOP["ebn0_db"] / 10))) / 10)


def test_reference_meets_the_rate_3_4_loopback_condition(m, o):
    """The oracle's TX and RX around chan_ref.channel, the numpy demapper quantised to int8 with
    qs = 8, ratematch_ref around fec_ref's decoder: at an information Eb/N0 of 4.5 dB the decoded
    errors of the 442 information bits are at most a tenth of what uncoded QPSK would make (995
    expected of 113152, so at most 100), and every frame whose CRC checks is free of errors."""
    C = LOOP
    assert loop_limit() == 100
    K, polys, nframes, nbits = C["K"], C["polys"], C["nframes"], C["nbits"]
    W, poly, init, xorout = C["crc"]
    sps, L = C["sps"], C["L"]
    n0 = loop_n0()
    bits = o.prng_bits(C["seed"], nframes * nbits).reshape(nframes, nbits)
    framed = R.attach(bits, W, poly, init, xorout)
    coded = fec_ref.encode(framed, K, polys)
    nm = coded.shape[1]
    assert nm == 928
    sent = R.tx(coded, C["pattern"], C["cols"])
    assert sent.shape[1] == 619 and abs(loop_rate() - 442 / 619) < 1e-15
    taps = m.rrc_taps(L, sps, 0.35)
    w = o.sample_freq(1, 4)
    x = o.tx_chain(o.new_phasor(o.QPSK, 0.0, 1.0), sent.reshape(-1), sps, taps, w, 0, flush_syms=(L - 1 + sps - 1) // sps)
    y, _ = chan_ref.channel(x, n0=n0, seed=C["noise_seed"])
    riq, _ = o.rx_chain(y.astype(np.float32), w, 0, o.MIX_COMPLEX, taps, sps, L - 1, None)
    lut = o.phasor_lut(o.new_phasor(o.QPSK, 0.0, 1.0))
    nsym = sent.size // 2
    llr = demap_i8(riq[:nsym], lut, C["qs"] / n0).reshape(nframes, -1)
    raw = int(np.sum((llr < 0) != (sent == 1)))
    p = 0.5 * math.erfc(math.sqrt(loop_rate() * 10.0 ** (C["ebn0_db"] / 10)))
    want, band = sent.size * p, 5 * math.sqrt(sent.size * p * (1 - p))
    got, _ = fec_ref.decode(fec_ref.quantise(R.rx(llr, nm, C["pattern"], C["cols"])), nbits + W, K, polys)
    ok = R.check(got, W, poly, init, xorout)
    wrong = (got[:, :nbits] != bits).sum(1)
    errors = int(wrong.sum())
    print(f"reference rate-3/4 loopback at {C['ebn0_db']} dB: {errors} decoded bit errors of {bits.size} (limit {loop_limit()}) in "
          f"{int((wrong > 0).sum())} frames, {int(ok.sum())} frames pass the CRC; {raw} raw errors of {sent.size}, expected "
          f"{want:.0f} +- {band:.0f}")
    assert errors <= loop_limit()
    assert not wrong[ok == 1].any()
    assert abs(raw - want) <= band


@pytest.mark.parametrize("pattern", [(1,), R.PUNCTURE_3_4])
def test_reference_meets_the_burst_condition(pattern):
    """64 noiseless frames, LLR +-64, the 24 transmitted LLRs at 200 .. 223 erased: with 32 columns
    every frame decodes, with one column (no interleaver) the CRC fails on almost every frame."""
    K, polys, nframes, nbits = 7, (0o171, 0o133), 64, 442
    W, poly, init, xorout = LOOP["crc"]
    rng = np.random.RandomState(24)
    bits = rng.randint(0, 2, (nframes, nbits)).astype(np.uint8)
    framed = R.attach(bits, W, poly, init, xorout)
    coded = fec_ref.encode(framed, K, polys)
    wrong = {}
    for cols in (32, 1):
        llr = (64 * (1 - 2 * R.tx(coded, pattern, cols).astype(np.int64))).astype(np.int8)
        llr[:, 200:224] = 0
        got, _ = fec_ref.decode(fec_ref.quantise(R.rx(llr, coded.shape[1], pattern, cols)), nbits + W, K, polys)
        ok = R.check(got, W, poly, init, xorout)
        assert np.array_equal(ok == 1, (got == framed).all(1))
        wrong[cols] = int((ok == 0).sum())
    print(f"burst of 24 erasures, pattern of {len(pattern)}: wrong frames of {nframes}: {wrong}")
    assert wrong[32] == 0 and wrong[1] > 0, wrong
