"""Rate matching and the frame check on the device against the restatement of
tests/ratematch_ref.py, bit for bit: RateMatch.tx and .rx over patterns, columns, frame lengths,
frame counts, dtypes and padded rows whose sentinels must survive; CRC.attach and .check over every
width, row lengths around the 64 chunks of a wave, the ok flags and single flipped bits; and each
capped grid at the smallest size of its loop's second trip. The stream ordering of the four entries
is tests/test_gpu_streams_ratematch.py."""
import functools
import os
import re

import numpy as np
import pytest

import ratematch_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

SENT = 0xA5
P64 = tuple(1 if i == 63 else 0 for i in range(64))            # weight 1: one value in 64 is kept
PATTERNS = {"none": (1,), "r23": R.PUNCTURE_2_3, "r34": R.PUNCTURE_3_4, "p64": P64}
COLS = (1, 7, 32, 255)
NMS = (1, 5, 63, 64, 65, 896, 897, 12288, 16384)
NFRAMES = (1, 3, 65)
CRCS = {8: (0x07, 0x5A, 0xC3), 16: (0x1021, 0xFFFF, 0x1D0F), 24: (0x864CFB, 0xB704CE, 0x00F00F), 32: (0x04C11DB7, 0xFFFFFFFF, 0xDEADBEEF)}
CRC_NBITS = (1, 7, 63, 64, 65, 458, 4097, 65536)
CRC_NFRAMES = (1, 3, 65, 257)
UINT = {"int8": np.uint8, "float16": np.uint16, "float32": np.uint32}
# -128 / -0 / NaN payloads / infinities, as the bits of each dtype
SPECIAL = {"int8": (0x80, 0x81, 0x7F, 0x00), "float16": (0x8000, 0x7E01, 0xFE55, 0x7C00, 0xFFFF, 0x0001),
           "float32": (0x80000000, 0x7FC00001, 0xFFABCDEF, 0x7F800000, 0xFFFFFFFF, 0x00000001)}


@functools.lru_cache(maxsize=None)
def _positions(pname, nm, C):
    return R.positions(PATTERNS[pname], nm, C)


def _consts():
    with open(os.path.join(ROOT, "rust-modem_amd", "csrc", "modem_ratematch.hip")) as f:
        return {k: int(v) for k, v in re.findall(r"constexpr int (k\w+) = (\d+)\s*[;,]", f.read())}


def _padded(torch, a, pad, fill=None):
    """a (numpy, 2-D) as the left columns of a wider device buffer: (the view of a's shape, the whole buffer)."""
    rng = np.random.RandomState(a.shape[1] + pad)
    whole = rng.randint(0, 256, (a.shape[0], (a.shape[1] + pad) * a.itemsize)).astype(np.uint8).view(a.dtype) if fill is None \
        else np.full((a.shape[0], a.shape[1] + pad), fill, a.dtype)
    whole[:, :a.shape[1]] = a
    t = torch.from_numpy(whole).cuda()
    return t[:, :a.shape[1]], t


def _sentinel_out(torch, nframes, ncols, pad, dtype):
    whole = torch.from_numpy(np.full((nframes, (ncols + pad) * np.dtype(dtype).itemsize), SENT, np.uint8).view(dtype)).cuda()
    return whole[:, :ncols], whole


def _bits_of(t):
    a = t.cpu().numpy()
    return a.view(UINT.get(a.dtype.name, a.dtype))


def _sentinels_intact(whole, ncols):
    a = whole.cpu().numpy()
    return bool((a[:, ncols:].view(np.uint8) == SENT).all())


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("pname", list(PATTERNS))
def test_tx_and_rx_equal_the_reference(m, torch_cuda, pname, cols):
    """Rows inside wider buffers: garbage behind the input rows, sentinels behind the output rows."""
    torch = torch_cuda
    pat = PATTERNS[pname]
    rm = m.RateMatch(pat, cols=cols)
    rng = np.random.RandomState(len(pat) * 1000 + cols)
    for nm in NMS:
        E = R.kept(pat, nm)
        if E == 0:                                                      # p64 below 64 mother indices
            with pytest.raises(m.ModemPanic):
                rm.kept(nm)
            continue
        assert rm.kept(nm) == E
        ms, pos = _positions(pname, nm, cols)
        assert len(ms) == E
        for nframes in NFRAMES:
            what = (pname, cols, nm, nframes)
            coded = rng.randint(0, 256, (nframes, nm)).astype(np.uint8)       # only bit 0 counts
            x, _ = _padded(torch, coded, 3)
            out, whole = _sentinel_out(torch, nframes, E, 5, np.uint8)
            assert rm.tx(x, out=out) is out
            want = np.zeros((nframes, E), np.uint8)
            want[:, pos] = coded[:, ms] & 1
            assert np.array_equal(out.cpu().numpy(), want), what
            assert _sentinels_intact(whole, E), what
            if nframes == 3:
                assert np.array_equal(rm.tx(torch.from_numpy(coded).cuda()).cpu().numpy(), want), what
            for name, ut in UINT.items():
                raw = rng.randint(0, 256, (nframes, E * np.dtype(ut).itemsize)).astype(np.uint8).view(ut)
                sp = SPECIAL[name]
                raw.reshape(-1)[::3] = np.array(sp, ut)[np.arange(raw.reshape(-1)[::3].size) % len(sp)]
                llr = raw.view(np.dtype(name))
                x, _ = _padded(torch, llr, 2)
                out, whole = _sentinel_out(torch, nframes, nm, 4, np.dtype(name))
                assert rm.rx(x, nm, out=out) is out
                want = np.zeros((nframes, nm), ut)
                want[:, ms] = raw[:, pos]
                assert np.array_equal(_bits_of(out), want), what + (name,)
                assert _sentinels_intact(whole, nm), what + (name,)


def test_rx_accepts_and_ignores_ok(m, torch_cuda):
    torch = torch_cuda
    rm = m.RateMatch(R.PUNCTURE_3_4, cols=32)
    llr = np.random.RandomState(5).randint(-128, 128, (5, 598)).astype(np.int8)
    ok = torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8, device="cuda")
    got = rm.rx(torch.from_numpy(llr).cuda(), 896, ok=ok).cpu().numpy()
    assert np.array_equal(got, R.rx(llr, 896, R.PUNCTURE_3_4, 32))
    assert tuple(m.RateMatch().rx(torch.empty((0, 10), dtype=torch.int8, device="cuda"), 10).shape) == (0, 10)
    assert tuple(m.RateMatch().tx(torch.empty((0, 10), dtype=torch.uint8, device="cuda")).shape) == (0, 10)
    x = torch.zeros((2, 100), dtype=torch.uint8, device="cuda")
    with pytest.raises(m.ModemPanic):
        m.RateMatch().tx(x[:, :60], out=x[:, 40:])                      # the byte ranges overlap
    with pytest.raises(ValueError):
        rm.rx(torch.zeros((2, 597), dtype=torch.int8, device="cuda"), 896)
    with pytest.raises(ValueError):
        rm.tx(torch.zeros((2, 896), dtype=torch.int8, device="cuda"))


@functools.lru_cache(maxsize=None)
def _crc_case(W, nbits):
    """The rows of the largest frame count (bytes with high bits set) and their attach, computed once."""
    poly, init, xorout = CRCS[W]
    rows = np.random.RandomState(W * 100003 + nbits).randint(0, 256, (max(CRC_NFRAMES), nbits)).astype(np.uint8)
    rows[0], rows[1] = 0, 0xFF
    return rows, R.attach(rows, W, poly, init, xorout)


@pytest.mark.parametrize("nbits", CRC_NBITS)
@pytest.mark.parametrize("W", list(CRCS))
def test_crc_attach_and_check_equal_the_reference(m, torch_cuda, W, nbits):
    torch = torch_cuda
    poly, init, xorout = CRCS[W]
    crc = m.CRC(W, poly, init, xorout)
    rows, framed = _crc_case(W, nbits)
    rng = np.random.RandomState(W + nbits)
    for nframes in CRC_NFRAMES:
        what = (W, nbits, nframes)
        x, _ = _padded(torch, rows[:nframes], 3)
        out, whole = _sentinel_out(torch, nframes, nbits + W, 6, np.uint8)
        assert crc.attach(x, out=out) is out
        assert np.array_equal(out.cpu().numpy(), framed[:nframes]), what
        assert _sentinels_intact(whole, nbits + W), what
        # check: high bits set in every byte (only bit 0 counts), rows inside a wider buffer
        dirty = framed[:nframes] | (rng.randint(0, 128, framed[:nframes].shape).astype(np.uint8) << 1)
        y, _ = _padded(torch, dirty, 2)
        assert crc.check(y).cpu().numpy().tolist() == [1] * nframes, what
        ones = torch.full((nframes,), 3, dtype=torch.uint8, device="cuda")
        assert crc.check(y, ok=ones).cpu().numpy().tolist() == [1] * nframes, what
        mix = (rng.randint(0, 3, nframes) * 5).astype(np.uint8)
        # one flipped bit per row at a random position, in every second row
        flip = np.arange(nframes) % 2 == 1
        at = rng.randint(0, nbits + W, nframes)
        bad = dirty.copy()
        bad[flip, at[flip]] ^= 1
        y, _ = _padded(torch, bad, 2)
        assert np.array_equal(crc.check(y).cpu().numpy(), (~flip).astype(np.uint8)), what
        want = R.check(bad, W, poly, init, xorout, ok=mix)
        assert np.array_equal(want, ((~flip) & (mix != 0)).astype(np.uint8))
        okt = torch.from_numpy(mix).cuda()
        assert np.array_equal(crc.check(y, ok=okt).cpu().numpy(), want), what
        assert crc.check(y, ok=okt, out=okt) is okt                     # in place
        assert np.array_equal(okt.cpu().numpy(), want), what


@pytest.mark.parametrize("W,poly,init,value", [(16, 0x1021, 0xFFFF, 0x29B1), (16, 0x1021, 0, 0x31C3), (32, 0x04C11DB7, 0xFFFFFFFF, 0x0376E6E7),
                                               (8, 0x07, 0, 0xF4), (24, 0x864CFB, 0xB704CE, 0x21CF02)])
def test_crc_check_values_on_the_device(m, torch_cuda, W, poly, init, value):
    msg = np.array([(ord(ch) >> (7 - i)) & 1 for ch in "123456789" for i in range(8)], np.uint8)[None, :]
    out = m.CRC(W, poly, init).attach(torch_cuda.from_numpy(msg).cuda()).cpu().numpy()[0]
    assert int("".join(str(b) for b in out[72:]), 2) == value
    assert m.CRC(W, poly, init).check(torch_cuda.empty((0, 72 + W), dtype=torch_cuda.uint8, device="cuda")).numel() == 0


def test_second_trip_of_every_capped_grid(m, torch_cuda):
    """rm_tx / rm_rx take kRmMaxGroup one-value frames per workgroup and trip, the CRC kCrcWaves frames:
    one frame more than kMaxBlocks workgroups hold gives the first workgroup a second trip. The
    shortest legal rows: Nm = 1, nbits = 1."""
    torch = torch_cuda
    c = _consts()
    assert c["kRmGroupElems"] >= c["kRmMaxGroup"] and c["kRmLds"] >= 4 * c["kRmMaxGroup"]     # Nm = 1: a group is kRmMaxGroup frames
    nframes = c["kRmMaxBlocks"] * c["kRmMaxGroup"] + 1
    rng = np.random.RandomState(2)
    rm = m.RateMatch((1,), cols=1)
    coded = rng.randint(0, 256, (nframes, 1)).astype(np.uint8)
    x, _ = _padded(torch, coded, 1)
    assert np.array_equal(rm.tx(x).cpu().numpy(), coded & 1)
    for name in UINT:
        llr = rng.randint(0, 256, (nframes, np.dtype(name).itemsize)).astype(np.uint8).view(np.dtype(name))
        x, _ = _padded(torch, llr, 1)
        assert np.array_equal(_bits_of(rm.rx(x, 1)), llr.view(UINT[name])), name
    nframes = c["kCrcMaxBlocks"] * c["kCrcWaves"] + 1
    crc = m.CRC.ccitt16()
    rows = rng.randint(0, 256, (nframes, 1)).astype(np.uint8)
    want = R.attach(rows, 16, 0x1021, 0xFFFF)
    got = crc.attach(torch.from_numpy(rows).cuda())
    assert np.array_equal(got.cpu().numpy(), want)
    flip = rng.randint(0, 2, nframes).astype(bool)
    got[torch.from_numpy(flip).cuda(), 5] ^= 1
    assert np.array_equal(crc.check(got).cpu().numpy(), (~flip).astype(np.uint8))
