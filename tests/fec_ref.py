"""Numpy restatement of the convolutional code of include/modem_hip.h ("Convolutional code"), for
the tests: the encoder, the quantiser of the decoder's input and the Viterbi decoder, with integer
metrics throughout, so the device is held to it bit for bit. Vectorised over frames and states, a
Python loop over steps."""
import numpy as np

START = -(1 << 30)
MAX_STEPS = {3: 4096, 4: 4096, 5: 4096, 6: 4096, 7: 4096, 8: 2048, 9: 1024}


def steps(K, nbits, tail=True):
    return nbits + (K - 1 if tail else 0)


def coded_bits(K, n, nbits, tail=True):
    return n * steps(K, nbits, tail)


def _parity(v):
    v = np.asarray(v, dtype=np.int64)
    p = np.zeros_like(v)
    while np.any(v):
        p ^= v & 1
        v = v >> 1
    return p


def encode(bits, K, polys, tail=True):
    """bits (nframes, nbits), bit 0 of each byte -> (nframes, n * T) uint8."""
    b = np.asarray(bits).astype(np.int64) & 1
    nframes, nbits = b.shape
    T, n = steps(K, nbits, tail), len(polys)
    b = np.concatenate([b, np.zeros((nframes, T - nbits), np.int64)], 1)
    out = np.zeros((nframes, T, n), np.uint8)
    s = np.zeros(nframes, np.int64)
    for t in range(T):
        reg = (b[:, t] << (K - 1)) | s
        for j, g in enumerate(polys):
            out[:, t, j] = _parity(reg & g)
        s = reg >> 1
    return out.reshape(nframes, T * n)


def quantise(v, qscale=1.0):
    """The q of a buffer of int8, float16 or float32 values."""
    v = np.asarray(v)
    if v.dtype == np.int8:
        return np.maximum(v.astype(np.int64), -127)
    p = v.astype(np.float32) * np.float32(qscale)                     # F16 widened exactly; one f32 product
    assert p.dtype == np.float32
    return np.rint(np.minimum(np.maximum(p, np.float32(-127.0)), np.float32(127.0))).astype(np.int64)


def trellis(K, polys):
    """p (2, S): the predecessors of every state; sg (2, n, S): 1 - 2 c of the branch from p[x]."""
    S = 1 << (K - 1)
    sn = np.arange(S, dtype=np.int64)
    b = sn >> (K - 2)
    p = np.stack([((sn << 1) & (S - 1)) | x for x in (0, 1)])
    sg = np.stack([np.stack([1 - 2 * _parity(((b << (K - 1)) | p[x]) & g) for g in polys]) for x in (0, 1)])
    return p, sg


def decode(q, nbits, K, polys, tail=True):
    """q (nframes, >= n * T) integers in [-127, 127] -> (bits (nframes, nbits) uint8, metric (nframes,) int32)."""
    q = np.asarray(q).astype(np.int64)
    nframes, n, S = q.shape[0], len(polys), 1 << (K - 1)
    T = steps(K, nbits, tail)
    assert q.shape[1] >= n * T and np.abs(q[:, :n * T]).max(initial=0) <= 127
    p, sg = trellis(K, polys)
    pm = np.full((nframes, S), START, np.int64)
    pm[:, 0] = 0
    dec = np.zeros((T, nframes, S), np.bool_)
    for t in range(T):
        qt = q[:, t * n:(t + 1) * n]
        m0 = pm[:, p[0]] + qt @ sg[0]
        m1 = pm[:, p[1]] + qt @ sg[1]
        dec[t] = m1 > m0                                             # ties keep x = 0
        pm = np.where(dec[t], m1, m0)
    assert pm.min() > -(1 << 31) and pm.max() < 1 << 29
    s = np.zeros(nframes, np.int64) if tail else np.argmax(pm, 1)     # the lowest index among equals
    rows = np.arange(nframes)
    metric = pm[rows, s].astype(np.int32)
    bits = np.zeros((nframes, T), np.uint8)
    for t in range(T - 1, -1, -1):
        bits[:, t] = s >> (K - 2)
        s = p[dec[t][rows, s].astype(np.int64), s]
    return bits[:, :nbits].copy(), metric


def correlation(code, q):
    """sum (1 - 2 c) q of codewords (m, L) against rows (r, L): (r, m)."""
    return np.asarray(q, np.int64) @ (1 - 2 * np.asarray(code, np.int64)).T
