"""Differential detector on the GPU (modem_diff_*, DiffDetector) against the float64 formula

    z[k]      = r[k] * conj(r[k-1])                     r[-1] = prev0
    c(s)      = z.re * lut[s, 0] + z.im * lut[s, 1]
    sym[k]    = argmax_s c(s)                           lowest index on ties
    llr[k, j] = scale * (max_{s: bit_j(s)=0} c(s) - max_{s: bit_j(s)=1} c(s)),   j = 0 the MSB

evaluated here in numpy float64 from the same f32 (or f16, widened) inputs and the table the library
returned (diff_lut(), pinned by test_noncoh_host.py).

f32 bound, element-wise, with u = 2^-24 and P = |r[k]| * |r[k-1]| in float64:
|got - ref| <= 2^-20 * |scale| * P + 1e-30. Each component of z carries <= 2uP (two products, one
sum), each c(s) <= (2 sqrt 2 + 2) uP (|lut[s]| <= 1 + u), the two maxima are 1-Lipschitz, the
subtraction and the scaling add <= 3uP: about 13uP, and 16uP leaves room for either FMA contraction
choice. Decisions equal the reference's wherever its best-minus-second margin exceeds twice that.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NSYMS = (1, 63, 64, 65, 257, 4099)
SIGMAS = (0.0, 0.15)
AMP, PHASE0 = 1.3, 0.785
SCALES = {1: 1.0, 2: 4.0, 3: 0.75, 4: 2.5}          # every one exact in f32


def shift_of(bps):
    return float(np.float32(2 * np.pi / (1 << bps)))


def phasor(m, bps):
    return m.DMPSK(bps, AMP, PHASE0, shift_of(bps))


@functools.lru_cache(maxsize=None)
def _lut_of(bps):
    import __graft_entry__ as graft
    return np.ascontiguousarray(phasor(graft.package(), bps).diff_lut(), np.float32)


def prev0_of():
    return np.array([AMP * np.cos(PHASE0), AMP * np.sin(PHASE0)], np.float32)     # what detector() passes


def synth(bps, n, sigma, seed=0):
    """(symbols drawn, r as (n, 2) f32): the DMPSK recurrence from PHASE0 in float64, plus noise."""
    rng = np.random.RandomState(0xD1FF + seed + 7919 * n + 131 * bps + int(1000 * sigma))
    s = rng.randint(0, 1 << bps, n)
    phi = PHASE0 + np.cumsum(s * np.float64(np.float32(shift_of(bps))))
    noise = rng.standard_normal((n, 2))
    r = AMP * np.stack([np.cos(phi), np.sin(phi)], 1) + sigma * noise
    return s.astype(np.uint8), np.ascontiguousarray(r.astype(np.float32))


def ref_diff(lut, iq, prev0, scale):
    """float64 (metrics c (n, M), sym, llr (n, bps), bound (n, 1), margin (n,)) of the module docstring."""
    r = np.asarray(iq).astype(np.float64)
    z = r[:, 0] + 1j * r[:, 1]
    zp = np.concatenate([[np.float64(prev0[0]) + 1j * np.float64(prev0[1])], z[:-1]])
    d = z * np.conj(zp)
    t = lut.astype(np.float64)
    c = d.real[:, None] * t[None, :, 0] + d.imag[:, None] * t[None, :, 1]
    M = len(lut)
    bps = M.bit_length() - 1
    s = np.arange(M)
    llr = np.empty((len(r), bps))
    for j in range(bps):
        one = ((s >> (bps - 1 - j)) & 1).astype(bool)
        llr[:, j] = float(scale) * (c[:, ~one].max(1) - c[:, one].max(1))
    P = np.abs(z) * np.abs(zp)
    bound = (2.0 ** -20 * abs(float(scale)) * P + 1e-30)[:, None]
    srt = np.sort(c, axis=1)
    return c, np.argmax(c, axis=1).astype(np.uint8), llr, bound, srt[:, -1] - srt[:, -2], P


@functools.lru_cache(maxsize=None)
def case(bps, n, sigma):
    """One input set and its reference, computed once and shared (treated as read-only)."""
    s, iq = synth(bps, n, sigma)
    _, sym, llr, bound, margin, P = ref_diff(_lut_of(bps), iq, prev0_of(), SCALES[bps])
    for a in (s, iq, sym, llr, bound, margin, P):
        a.setflags(write=False)
    return s, iq, sym, llr, bound, margin, P


def _check_f32(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(np.max(err / bound))
    print(f"{what}: max |got-ref| / bound = {worst:.3f}, max |ref| = {np.abs(ref).max():.4g}")
    assert got.shape == ref.shape
    assert np.all(err <= bound), f"{what}: {int(np.sum(err > bound))} of {err.size} outside the bound (worst {worst:.3f}x)"


def _check_sym(got, ref_sym, margin, P, what):
    clear = margin > 2 * 2.0 ** -20 * P
    print(f"{what}: {int((~clear).sum())} of {len(clear)} symbols within the decision margin")
    assert (~clear).mean() <= 0.01
    assert got.shape == ref_sym.shape and got.dtype == np.uint8
    assert np.array_equal(got[clear], ref_sym[clear]), what


# ----------------------------------------------------------------------------- parity ----
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("n", NSYMS)
@pytest.mark.parametrize("bps", [1, 2, 3, 4])
def test_parity_with_float64(m, torch_cuda, bps, n, sigma):
    torch = torch_cuda
    drawn, iq, rsym, rllr, bound, margin, P = case(bps, n, sigma)
    det = phasor(m, bps).detector()
    assert np.array_equal(det.prev0, prev0_of()) and np.array_equal(det.lut, _lut_of(bps))
    sym, llr = det.process(torch.tensor(iq, device="cuda"), SCALES[bps])
    assert sym.dtype == torch.uint8 and llr.dtype == torch.float32 and tuple(llr.shape) == (n, bps)
    what = f"diff bps {bps} n {n} sigma {sigma}"
    _check_f32(llr.cpu().numpy(), rllr, bound, what)
    _check_sym(sym.cpu().numpy(), rsym, margin, P, what)
    if sigma == 0.0:
        assert np.array_equal(sym.cpu().numpy(), drawn)
        assert np.array_equal(rsym, drawn)


def test_table_and_default_prev0(m, torch_cuda):
    """A hand-made table and no prev0: r[-1] = (1, 0)."""
    torch = torch_cuda
    _, iq, *_ = case(3, 257, 0.15)
    lut = _lut_of(3)
    det = m.DiffDetector(lut)
    sym, llr = det.process(torch.tensor(iq, device="cuda"), 0.75)
    _, rsym, rllr, bound, margin, P = ref_diff(lut, iq, (1.0, 0.0), 0.75)
    _check_f32(llr.cpu().numpy(), rllr, bound, "diff table, prev0 default")
    _check_sym(sym.cpu().numpy(), rsym, margin, P, "diff table, prev0 default")


@pytest.mark.parametrize("bps", [1, 2, 4])
def test_zero_points_tie_to_symbol_zero(m, torch_cuda, bps):
    torch = torch_cuda
    iq = np.array([[0.7, -0.4], [0, 0], [0, 0], [1.1, 0.3], [0.2, 0.9]], np.float32)
    det = phasor(m, bps).detector()
    sym, llr = det.process(torch.tensor(iq, device="cuda"), 3.0)
    sym, llr = sym.cpu().numpy(), llr.cpu().numpy()
    assert np.array_equal(sym[1:4], [0, 0, 0])            # z = 0 at k = 1, 2 and (r[2] = 0) at 3
    assert np.all(llr[1:4] == 0)
    assert np.any(llr[0] != 0) and np.any(llr[4] != 0)


# ------------------------------------------------------------------------- dtypes ----
def test_f16_input(m, torch_cuda):
    """f16 I/Q is widened exactly: the reference uses the f16 values as float64."""
    torch = torch_cuda
    _, iq, *_ = case(3, 4099, 0.15)
    iq16 = iq.astype(np.float16)
    det = phasor(m, 3).detector(in_dtype=m.DTYPE_F16)
    sym, llr = det.process(torch.tensor(iq16, device="cuda"), 0.75)
    _, rsym, rllr, bound, margin, P = ref_diff(_lut_of(3), iq16, prev0_of(), 0.75)
    _check_f32(llr.cpu().numpy(), rllr, bound, "diff f16 in")
    _check_sym(sym.cpu().numpy(), rsym, margin, P, "diff f16 in")
    with pytest.raises(ValueError):
        det.process(torch.tensor(iq, device="cuda"), 0.75)


F16_SCALE = 40000.0


def test_f16_output_saturates(m, torch_cuda):
    """Round to nearest, saturating to +-65504, never inf: bound = the f32 bound + 2^-11 |ref| +
    2^-25 below 0.99 * 65504; exactly +-65504 where |ref| > 70000; in between (where the two rules
    meet) a finite value of at least 0.98 * 65504 in magnitude with the reference's sign."""
    torch = torch_cuda
    _, iq, *_ = case(2, 4099, 0.15)
    _, _, ref, bound, _, _ = ref_diff(_lut_of(2), iq, prev0_of(), F16_SCALE)
    a = np.abs(ref)
    sat, inside = a > 70000, a < 0.99 * 65504
    print(f"diff f16 out: {int(sat.sum())} saturating, {int(inside.sum())} in range, max |ref| {a.max():.4g}")
    assert sat.sum() >= 8 and inside.sum() >= 8
    assert np.any(ref[sat] > 0) and np.any(ref[sat] < 0)
    det = phasor(m, 2).detector(llr_dtype=m.DTYPE_F16)
    _, got = det.process(torch.tensor(iq, device="cuda"), F16_SCALE)
    assert got.dtype == torch.float16
    g = got.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(g))
    assert np.array_equal(g[sat], np.sign(ref[sat]) * 65504.0)
    err = np.abs(g - ref)[inside]
    lim = (np.broadcast_to(bound, ref.shape) + 2.0 ** -11 * a + 2.0 ** -25)[inside]
    print(f"diff f16 out: max err / bound = {np.max(err / lim):.3f}")
    assert np.all(err <= lim)
    mid = ~(sat | inside)
    assert np.all(np.abs(g[mid]) >= 0.98 * 65504) and np.all(np.sign(g[mid]) == np.sign(ref[mid]))


I8_SCALE = 64.0


def test_i8_output(m, torch_cuda):
    """q = rint(clip(ref, -127, 127)): |got - q| <= 1 everywhere, got == q wherever ref lies
    further than the f32 bound from a half-integer (at most 1 % of the elements lie closer)."""
    torch = torch_cuda
    _, iq, *_ = case(2, 4099, 0.15)
    _, _, ref, bound, _, _ = ref_diff(_lut_of(2), iq, prev0_of(), I8_SCALE)
    q = np.rint(np.clip(ref, -127, 127))
    near = np.abs(ref - (np.floor(ref) + 0.5)) <= bound
    print(f"diff i8 out: ref in [{ref.min():.4g}, {ref.max():.4g}], {near.mean() * 100:.3f} % near a half-integer")
    assert ref.min() < -127.5 and ref.max() > 127.5 and np.any(np.abs(ref) < 100)
    assert near.mean() <= 0.01
    det = phasor(m, 2).detector(llr_dtype=m.DTYPE_I8)
    _, got = det.process(torch.tensor(iq, device="cuda"), I8_SCALE)
    assert got.dtype == torch.int8 and tuple(got.shape) == ref.shape
    g = got.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(g - q) <= 1)
    assert np.array_equal(g[~near], q[~near])
    assert g.min() == -127 and g.max() == 127


# ------------------------------------------------------------------ chunks and buffers ----
_DT = {"f32": ("DTYPE_F32", "float32"), "f16": ("DTYPE_F16", "float16"), "i8": ("DTYPE_I8", "int8")}


@pytest.mark.parametrize("out_dtype", ["f32", "f16", "i8"])
@pytest.mark.parametrize("bps", [1, 3, 4])
def test_cuts_views_and_host_pointers_are_bitwise_identical(m, torch_cuda, bps, out_dtype):
    """One 4099-symbol call; the cuts 1 + 0 + 999 + 3099 (the carried point across calls); output
    views that start one element into their buffers (the narrower store path); host pointers."""
    torch = torch_cuda
    dt, tdt = getattr(m, _DT[out_dtype][0]), getattr(torch, _DT[out_dtype][1])
    _, iq, *_ = case(bps, 4099, 0.15)
    n, scale = len(iq), 20.0
    x = torch.tensor(iq, device="cuda")
    mk = lambda: phasor(m, bps).detector(llr_dtype=dt)          # noqa: E731
    wsym, wllr = mk().process(x, scale)
    ws, wl = wsym.cpu().numpy(), wllr.cpu().numpy()
    assert np.count_nonzero(wl) > wl.size // 2 and len(np.unique(ws)) == 1 << bps

    det = mk()
    csym = torch.zeros(n, dtype=torch.uint8, device="cuda")
    cllr = torch.zeros((n, bps), dtype=tdt, device="cuda")
    a = 0
    for k in (1, 0, 999, 3099):
        det.process(x[a:a + k], scale, out_sym=csym[a:a + k], out_llr=cllr[a:a + k])
        a += k
    assert a == n
    assert np.array_equal(ws, csym.cpu().numpy())
    assert np.array_equal(wl.view(np.uint8), cllr.cpu().numpy().view(np.uint8))

    sbuf = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    lbuf = torch.zeros(n * bps + 1, dtype=tdt, device="cuda")
    sview, lview = sbuf[1:], lbuf[1:].view(n, bps)
    assert lview.data_ptr() % 16 == wllr.element_size() and wllr.data_ptr() % 16 == 0
    mk().process(x, scale, out_sym=sview, out_llr=lview)
    assert np.array_equal(ws, sview.cpu().numpy())
    assert np.array_equal(wl.view(np.uint8), lview.cpu().numpy().view(np.uint8))
    assert sbuf[0].item() == 0 and lbuf[0].item() == 0

    hsym, hllr = mk().process(np.array(iq), scale)
    assert isinstance(hsym, np.ndarray) and isinstance(hllr, np.ndarray) and hllr.shape == (n, bps)
    assert hsym.dtype == np.uint8 and hllr.dtype == np.dtype(_DT[out_dtype][1])
    assert np.array_equal(ws, hsym)
    assert np.array_equal(wl.view(np.uint8), hllr.view(np.uint8))


def test_capacity_and_bad_scale(m, torch_cuda):
    """CAPACITY writes nothing and leaves the carried point alone: the next call continues the
    stream as if the refused call had not been made."""
    torch = torch_cuda
    _, iq, *_ = case(2, 257, 0.15)
    x = torch.tensor(iq, device="cuda")
    wsym, wllr = phasor(m, 2).detector().process(x, 1.0)
    det = phasor(m, 2).detector()
    s0, l0 = det.process(x[:100], 1.0)
    osym = torch.full((156,), 9, dtype=torch.uint8, device="cuda")
    ollr = torch.full((157, 2), -7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(m.ModemError) as e:
        det.process(x[100:], 1.0, out_sym=osym, out_llr=ollr)
    assert e.value.status == m.ERR_CAPACITY
    ollr2 = torch.full((156, 2), -7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(m.ModemError) as e:
        det.process(x[100:], 1.0, out_llr=ollr2)
    assert e.value.status == m.ERR_CAPACITY
    torch.cuda.synchronize()
    assert bool(torch.all(osym == 9)) and bool(torch.all(ollr == -7.0)) and bool(torch.all(ollr2 == -7.0))
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(m.ModemPanic):
            det.process(x[100:], bad)
    es, el = det.process(x[:0], 1.0)                         # nsym == 0: OK, no launch
    assert tuple(es.shape) == (0,) and tuple(el.shape) == (0, 2)
    s1, l1 = det.process(x[100:], 1.0)
    assert torch.equal(torch.cat([s0, s1]), wsym) and torch.equal(torch.cat([l0, l1]), wllr)
    with pytest.raises(ValueError):
        det.process(x, 1.0, out_llr=torch.zeros((257, 2), dtype=torch.float16, device="cuda"))


# --------------------------------------------------------------------------- loopback ----
def _loopback(m, torch, ph, bits_np, chunks):
    sps, bps = 4, ph.bits_per_symbol()
    fr = m.Freq(1000, 10000)
    tx = m.DigitalModulator(m.Carrier(fr), ph, sps, None)
    rx = m.DemodulatorRx(m.Carrier(fr), np.ones(4, np.float32) / 4, decim=sps, decim_offset=sps - 1, mix=m.MIX_COMPLEX)
    det = ph.detector()
    bits = torch.tensor(bits_np, device="cuda")
    syms, llrs = [], []
    a = 0
    for nb in chunks:
        y = tx.process(bits[a:a + nb])
        a += nb
        riq, _ = rx.process(y, want_sym=False)
        s, l = det.process(riq, 1.0)
        syms.append(s)
        llrs.append(l)
    assert a == len(bits_np)
    return torch.cat(syms).cpu().numpy(), torch.cat(llrs).cpu().numpy().reshape(-1, bps)


@pytest.mark.parametrize("name", ["dqpsk", "dbpsk"])
def test_loopback_recovers_the_bits(m, torch_cuda, name):
    """TX (sample-and-hold, mixed I/Q) -> boxcar matched filter at the symbol instants -> the
    differential detector: every decision is the symbol sent and llr < 0 the bits sent, in one
    call and with the TX and the detector driven in three ragged chunks."""
    torch = torch_cuda
    mk = {"dqpsk": lambda: m.DMPSK(2, 1.0, 0.7853982, 1.5707964), "dbpsk": lambda: m.DMPSK(1, 1.0, 0.7853982, 3.1415927)}[name]
    bps, nsym = mk().bits_per_symbol(), 2048
    bits_np = np.random.RandomState(0x5EED + bps).randint(0, 2, nsym * bps).astype(np.uint8)
    sent = (bits_np.reshape(-1, bps).astype(np.int64) @ (1 << np.arange(bps)[::-1])).astype(np.uint8)
    for chunks in ([nsym * bps], [bps * 700 + 1, bps * 5 - 1 if bps > 1 else 3, None]):
        chunks = [c if c is not None else nsym * bps - sum(x for x in chunks if x is not None) for c in chunks]
        sym, llr = _loopback(m, torch, mk(), bits_np, chunks)
        assert sym.shape == (nsym,) and llr.shape == (nsym, bps)
        assert np.array_equal(sym, sent)
        assert not np.any(llr == 0)
        assert np.array_equal((llr < 0).astype(np.uint8).reshape(-1), bits_np)
