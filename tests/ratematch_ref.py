"""Numpy restatement of include/modem_hip.h, "Rate matching and frame check": the rank of a kept
mother index, the pruned block interleaver, puncturing and its inverse, and the bit-serial CRC.
Straight from the definitions, one Python step per definition step; nothing here is shared with the
product's code."""
import numpy as np

PUNCTURE_2_3 = (1, 1, 1, 0)
PUNCTURE_3_4 = (1, 1, 1, 0, 0, 1)


def is_kept(pattern, m):
    return pattern[m % len(pattern)] == 1


def rank(pattern, m):
    """j = (m / P) * w + #{i < m mod P : pattern[i] = 1} (for a kept m)."""
    P = len(pattern)
    return (m // P) * sum(pattern) + sum(1 for i in range(m % P) if pattern[i] == 1)


def kept(pattern, nm):
    """E: the kept indices below nm, counted one by one."""
    return sum(1 for m in range(nm) if is_kept(pattern, m))


def pi(j, E, C):
    rows = -(-E // C)
    cl = E - (rows - 1) * C
    r, c = divmod(j, C)
    return c * rows + r - max(0, c - cl)


def positions(pattern, nm, C):
    """(the kept m, their transmitted positions pi(rank(m)))."""
    E = kept(pattern, nm)
    ms = [m for m in range(nm) if is_kept(pattern, m)]
    return np.array(ms, np.int64), np.array([pi(rank(pattern, m), E, C) for m in ms], np.int64)


def tx(bits, pattern, C):
    """(nframes, nm) -> (nframes, E): out[f][pi(rank(m))] = in[f][m] & 1."""
    bits = np.asarray(bits)
    ms, pos = positions(pattern, bits.shape[1], C)
    out = np.zeros((bits.shape[0], len(ms)), np.uint8)
    out[:, pos] = bits[:, ms] & 1
    return out


def rx(llr, nm, pattern, C):
    """(nframes, E) -> (nframes, nm) of the same dtype: the values as they are, a punctured m all bits zero."""
    llr = np.asarray(llr)
    ms, pos = positions(pattern, nm, C)
    assert llr.shape[1] == len(ms)
    out = np.zeros((llr.shape[0], nm), llr.dtype)
    out[:, ms] = llr[:, pos]
    return out


def crc(bits, W, poly, init=0, xorout=0):
    """The CRC of one row of bits (bit 0 of each value), by the definition's step."""
    reg = init
    for b in np.asarray(bits).reshape(-1):
        fb = (reg >> (W - 1)) ^ (int(b) & 1)
        reg = (reg << 1) % (1 << W)
        if fb:
            reg ^= poly
    return reg ^ xorout


def crc_rows(bits, W, poly, init=0, xorout=0):
    """The same for every row at once: (nframes, nbits) -> nframes Python-int-valued uint64."""
    b = np.asarray(bits).astype(np.uint64) & np.uint64(1)
    reg = np.full(b.shape[0], init, np.uint64)
    top, mask, p = np.uint64(W - 1), np.uint64((1 << W) - 1), np.uint64(poly)
    for i in range(b.shape[1]):
        fb = (reg >> top) ^ b[:, i]
        reg = (reg << np.uint64(1)) & mask
        reg = np.where(fb == 1, reg ^ p, reg)
    return reg ^ np.uint64(xorout)


def attach(bits, W, poly, init=0, xorout=0):
    """(nframes, nbits) -> (nframes, nbits + W): the bits & 1, then the CRC, MSB first."""
    bits = np.asarray(bits)
    c = crc_rows(bits, W, poly, init, xorout)
    tail = ((c[:, None] >> np.arange(W - 1, -1, -1, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
    return np.concatenate([(bits & 1).astype(np.uint8), tail], 1)


def check(bits, W, poly, init=0, xorout=0, ok=None):
    """(nframes, nbits + W) -> ok' uint8: the CRC of the first nbits equals the trailing W bits, and ok (if any) != 0."""
    bits = np.asarray(bits)
    nbits = bits.shape[1] - W
    c = crc_rows(bits[:, :nbits], W, poly, init, xorout)
    got = np.zeros(bits.shape[0], np.uint64)
    for i in range(W):
        got = (got << np.uint64(1)) | (bits[:, nbits + i].astype(np.uint64) & np.uint64(1))
    good = c == got
    if ok is not None:
        good &= np.asarray(ok) != 0
    return good.astype(np.uint8)
