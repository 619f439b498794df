"""Tone-bank energy detector on the GPU (modem_fsk_*, ToneDetector) against the float64 formula

    S[k, m]   = sum_{i < sps} x[k*sps + i] * e^{-j omega[m] i}
    E[k, m]   = |S[k, m]|^2
    sym[k]    = argmax_m E[k, m]                        lowest index on ties
    llr[k, j] = scale * (max_{m: bit_j(m)=0} E - max_{m: bit_j(m)=1} E),   j = 0 the MSB

evaluated here in numpy float64 from the same f32 (or f16, widened) samples with exact twiddles of
the f32 omega the library returned (tones(), pinned by test_noncoh_host.py).

Bounds, with u = 2^-24 and A = sum_i |x[k*sps + i]|: the products and the table rounding give
<= 3uA per component of S, an accumulation in any order <= (sps - 1) uA, so |dS| <= sqrt 2 (sps + 2) uA;
dE <= 2 |S| |dS| + 3uE with |S| <= A:  bE = (3 sps + 16) u A^2  per energy;
llr: |scale| * (2 bE + 2^-22 max_m E). Decisions equal the reference's wherever its margin exceeds 2 bE.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CARRIER = 0.3
# name -> (bps, sps, phasor constructor)
CASES = {
    "bfsk_4": (1, 4, lambda m: m.BFSK(m.Freq(1, 4), 1.0)),
    "mfsk2_8": (2, 8, lambda m: m.MFSK(2, m.Freq(1, 16), 1.0, "increase")),
    "mfsk4_16": (4, 16, lambda m: m.MFSK(4, m.Freq(1, 32), 1.0, "default")),
    "mfsk3_45": (3, 45, lambda m: m.MFSK(3, m.Freq(120, 10000), 1.0, "default")),   # non-orthogonal, odd sps
    "mfsk8_256": (8, 256, lambda m: m.MFSK(8, m.Freq(1, 512), 1.0, "increase")),    # the table limit
}
NSYMS = {name: (65,) if name == "mfsk8_256" else (1, 63, 65, 4099) for name in CASES}
SCALES = {"bfsk_4": 1.0, "mfsk2_8": 0.5, "mfsk4_16": 0.25, "mfsk3_45": 2.0, "mfsk8_256": 0.125}
PARITY = [(name, n, sigma) for name in CASES for n in NSYMS[name] for sigma in (0.0, 0.5)]


@functools.lru_cache(maxsize=None)
def omega_of(name):
    import __graft_entry__ as graft
    return np.ascontiguousarray(CASES[name][2](graft.package()).tones(CARRIER), np.float32)


def synth(omega, sps, n, sigma, seed=0):
    """(tones drawn, x as (n*sps, 2) f32): one tone per symbol at a random phase, plus noise."""
    rng = np.random.RandomState(0xF5C + seed + 7919 * n + 31 * sps + int(1000 * sigma))
    s = rng.randint(0, len(omega), n)
    theta = rng.uniform(0, 2 * np.pi, n)
    ph = omega.astype(np.float64)[s][:, None] * np.arange(sps)[None, :] + theta[:, None]
    x = np.stack([np.cos(ph), np.sin(ph)], 2) + sigma * rng.standard_normal((n, sps, 2))
    return s.astype(np.uint8), np.ascontiguousarray(x.reshape(n * sps, 2).astype(np.float32))


def ref_fsk(omega, sps, x, scale):
    """float64 (E (n, M), sym, llr (n, bps), bE (n, 1), llr bound (n, 1), margin (n,)) of the docstring."""
    x = np.asarray(x).astype(np.float64)
    n = len(x) // sps
    z = (x[: n * sps, 0] + 1j * x[: n * sps, 1]).reshape(n, sps)
    W = np.exp(-1j * np.arange(sps)[:, None] * omega.astype(np.float64)[None, :])
    S = z @ W
    E = S.real ** 2 + S.imag ** 2
    M = len(omega)
    bps = M.bit_length() - 1
    idx = np.arange(M)
    llr = np.empty((n, bps))
    for j in range(bps):
        one = ((idx >> (bps - 1 - j)) & 1).astype(bool)
        llr[:, j] = float(scale) * (E[:, ~one].max(1) - E[:, one].max(1))
    A = np.abs(z).sum(1)
    bE = ((3 * sps + 16) * U * A ** 2)[:, None]
    bl = abs(float(scale)) * (2 * bE + 2.0 ** -22 * E.max(1)[:, None]) + 1e-30
    srt = np.sort(E, axis=1)
    return E, np.argmax(E, axis=1).astype(np.uint8), llr, bE, bl, srt[:, -1] - srt[:, -2]


@functools.lru_cache(maxsize=None)
def case(name, n, sigma):
    """One input set and its reference, computed once and shared (treated as read-only)."""
    bps, sps, _ = CASES[name]
    s, x = synth(omega_of(name), sps, n, sigma)
    out = (s, x) + ref_fsk(omega_of(name), sps, x, SCALES[name])
    for a in out:
        a.setflags(write=False)
    return out


def _check(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{what}: max |got-ref| / bound = {worst:.3f}, max |ref| = {np.abs(ref).max():.4g}")
    assert got.shape == ref.shape
    assert np.all(err <= bound), f"{what}: {int(np.sum(err > bound))} of {err.size} outside the bound (worst {worst:.3f}x)"


def _check_sym(got, rsym, margin, bE, what):
    clear = margin > 2 * bE[:, 0]
    print(f"{what}: {int((~clear).sum())} of {len(clear)} symbols within the decision margin")
    assert (~clear).mean() <= 0.01
    assert got.shape == rsym.shape and got.dtype == np.uint8
    assert np.array_equal(got[clear], rsym[clear]), what


def _detector(m, name, **kw):
    bps, sps, mk = CASES[name]
    return mk(m).detector(sps, CARRIER, **kw)


# ----------------------------------------------------------------------------- parity ----
@pytest.mark.parametrize("name,n,sigma", PARITY)
def test_parity_with_float64(m, torch_cuda, name, n, sigma):
    torch = torch_cuda
    bps, sps, _ = CASES[name]
    drawn, x, E, rsym, rllr, bE, bl, margin = case(name, n, sigma)
    det = _detector(m, name)
    assert np.array_equal(det.omega, omega_of(name))
    sym, llr, en = det.process(torch.tensor(x, device="cuda"), SCALES[name], want_energy=True)
    assert tuple(sym.shape) == (n,) and tuple(llr.shape) == (n, bps) and tuple(en.shape) == (n, 1 << bps)
    assert sym.dtype == torch.uint8 and llr.dtype == torch.float32 and en.dtype == torch.float32
    what = f"fsk {name} n {n} sigma {sigma}"
    _check(en.cpu().numpy(), E, np.broadcast_to(bE, E.shape), what + " energy")
    _check(llr.cpu().numpy(), rllr, np.broadcast_to(bl, rllr.shape), what + " llr")
    _check_sym(sym.cpu().numpy(), rsym, margin, bE, what)
    if sigma == 0.0:
        assert np.array_equal(sym.cpu().numpy(), drawn)
        assert np.array_equal(rsym, drawn)


@pytest.mark.parametrize("name", ["bfsk_4", "mfsk4_16", "mfsk3_45", "mfsk8_256"])
def test_all_zero_symbol(m, torch_cuda, name):
    torch = torch_cuda
    bps, sps, _ = CASES[name]
    _, x, *_ = case(name, 65, 0.5)
    x = x[: 5 * sps].copy()
    x[2 * sps: 3 * sps] = 0
    sym, llr, en = _detector(m, name).process(torch.tensor(x, device="cuda"), 3.0, want_energy=True)
    sym, llr, en = sym.cpu().numpy(), llr.cpu().numpy(), en.cpu().numpy()
    assert sym[2] == 0 and np.all(en[2] == 0) and np.all(llr[2] == 0)
    assert np.all(en[[0, 1, 3, 4]].max(1) > 0) and np.any(llr[3] != 0)


def test_explicit_tones_without_a_phasor(m, torch_cuda):
    torch = torch_cuda
    name = "mfsk3_45"
    _, x, E, rsym, rllr, bE, bl, margin = case(name, 63, 0.5)
    det = m.ToneDetector(omega_of(name), 45)
    sym, llr = det.process(torch.tensor(x, device="cuda"), SCALES[name])
    _check(llr.cpu().numpy(), rllr, np.broadcast_to(bl, rllr.shape), "fsk explicit tones llr")
    _check_sym(sym.cpu().numpy(), rsym, margin, bE, "fsk explicit tones")


# -------------------------------------------------------------------------- streaming ----
_DT = {"f32": ("DTYPE_F32", "float32"), "f16": ("DTYPE_F16", "float16"), "i8": ("DTYPE_I8", "int8")}
STREAM_SCALE = {"bfsk_4": 4.0, "mfsk2_8": 1.0, "mfsk4_16": 0.25, "mfsk3_45": 0.05, "mfsk8_256": 0.001}


@pytest.mark.parametrize("out_dtype", ["f32", "f16", "i8"])
@pytest.mark.parametrize("name,n", [("bfsk_4", 4099), ("mfsk2_8", 4099), ("mfsk4_16", 4099), ("mfsk3_45", 4099),
                                    ("mfsk8_256", 65)])
def test_cuts_views_and_host_pointers_are_bitwise_identical(m, torch_cuda, name, n, out_dtype):
    """One call; the same samples cut at the offsets [1, 0, sps-1, sps+1, rest] (the carried samples
    across calls, a call without a whole symbol, a call without samples); a misaligned LLR view;
    host pointers. The input ends with a partial symbol, which stays in the handle."""
    torch = torch_cuda
    bps, sps, _ = CASES[name]
    dt, tdt = getattr(m, _DT[out_dtype][0]), getattr(torch, _DT[out_dtype][1])
    _, x, *_ = case(name, n, 0.5)
    tail = max(1, sps // 3)
    xs = np.ascontiguousarray(np.concatenate([x, x[:tail]]))          # n symbols and a partial one
    xd = torch.tensor(xs, device="cuda")
    scale = STREAM_SCALE[name]
    mk = lambda: _detector(m, name, llr_dtype=dt)                  # noqa: E731
    whole = mk()
    wsym, wllr, wen = whole.process(xd, scale, want_energy=True)
    assert tuple(wsym.shape) == (n,) and whole.nsymbols(sps - tail) == 1
    ws, wl, we = wsym.cpu().numpy(), wllr.cpu().numpy(), wen.cpu().numpy()
    assert np.count_nonzero(wl) > wl.size // 2

    det = mk()
    parts, a = [], 0
    for k in (1, 0, sps - 1, sps + 1, len(xs) - 2 * sps - 1):
        parts.append(det.process(xd[a:a + k], scale, want_energy=True))
        a += k
    assert a == len(xs)
    assert [int(p[0].shape[0]) for p in parts[:4]] == [0, 0, 1, 1]
    assert sum(int(p[0].shape[0]) for p in parts) == len(xs) // sps == n
    assert np.array_equal(ws, torch.cat([p[0] for p in parts]).cpu().numpy())
    assert np.array_equal(wl.view(np.uint8), torch.cat([p[1] for p in parts]).cpu().numpy().view(np.uint8))
    assert np.array_equal(we.view(np.uint8), torch.cat([p[2] for p in parts]).cpu().numpy().view(np.uint8))
    # the partial symbol is still there: completing it gives one more symbol in both handles
    more = torch.tensor(x[tail:sps], device="cuda")
    s1, l1 = whole.process(more, scale)
    s2, l2 = det.process(more, scale)
    assert tuple(s1.shape) == (1,) and torch.equal(s1, s2) and torch.equal(l1, l2)
    assert s1.cpu().numpy()[0] == ws[0] and np.array_equal(l1.cpu().numpy().view(np.uint8)[0], wl.view(np.uint8)[0])

    lbuf = torch.zeros(n * bps + 1, dtype=tdt, device="cuda")
    lview = lbuf[1:].view(n, bps)
    assert lview.data_ptr() % 16 == wllr.element_size()
    vsym, _ = mk().process(xd, scale, out_llr=lview)
    assert np.array_equal(ws, vsym.cpu().numpy())
    assert np.array_equal(wl.view(np.uint8), lview.cpu().numpy().view(np.uint8))
    assert lbuf[0].item() == 0

    hsym, hllr, hen = mk().process(xs, scale, want_energy=True)
    assert all(isinstance(h, np.ndarray) for h in (hsym, hllr, hen)) and hllr.dtype == np.dtype(_DT[out_dtype][1])
    assert np.array_equal(ws, hsym)
    assert np.array_equal(wl.view(np.uint8), hllr.view(np.uint8))
    assert np.array_equal(we.view(np.uint8), hen.view(np.uint8))


# ------------------------------------------------------------------ limits and errors ----
def test_table_limit(m, torch_cuda):
    """sps * 2^bps = 65536 creates a detector (and detects: every chunk of a 32768-sample symbol);
    131072 is refused."""
    torch = torch_cuda
    omega = np.array([0.3, 0.3 + 2 * np.pi / 1024], np.float32)
    sps = 32768
    det = m.ToneDetector(omega, sps)
    drawn, x = synth(omega, sps, 3, 0.5)
    E, rsym, rllr, bE, bl, margin = ref_fsk(omega, sps, x, 1e-6)
    sym, llr, en = det.process(torch.tensor(x, device="cuda"), 1e-6, want_energy=True)
    _check(en.cpu().numpy(), E, np.broadcast_to(bE, E.shape), "fsk sps 32768 energy")
    _check(llr.cpu().numpy(), rllr, np.broadcast_to(bl, rllr.shape), "fsk sps 32768 llr")
    assert np.array_equal(sym.cpu().numpy(), drawn)
    m.ToneDetector(omega_of("mfsk8_256"), 256)
    for om, s in ((omega, 65536), (omega_of("mfsk8_256"), 512)):
        with pytest.raises(m.ModemError) as e:
            m.ToneDetector(om, s)
        assert e.value.status == m.ERR_UNSUPPORTED


def test_capacity_and_bad_scale(m, torch_cuda):
    """CAPACITY writes nothing and leaves the carried samples alone: the next call continues the
    stream as if the refused call had not been made."""
    torch = torch_cuda
    name, sps = "mfsk2_8", 8
    _, x, *_ = case(name, 63, 0.5)
    xd = torch.tensor(x, device="cuda")
    wsym, wllr = _detector(m, name).process(xd, 1.0)
    det = _detector(m, name)
    cut = 20 * sps + 3
    s0, l0 = det.process(xd[:cut], 1.0)
    assert tuple(s0.shape) == (20,)
    osym = torch.full((42,), 9, dtype=torch.uint8, device="cuda")
    ollr = torch.full((43, 2), -7.0, dtype=torch.float32, device="cuda")
    oen = torch.full((43, 4), -7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(m.ModemError) as e:
        det.process(xd[cut:], 1.0, out_sym=osym, out_llr=ollr, out_energy=oen)
    assert e.value.status == m.ERR_CAPACITY
    torch.cuda.synchronize()
    assert bool(torch.all(osym == 9)) and bool(torch.all(ollr == -7.0)) and bool(torch.all(oen == -7.0))
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(m.ModemPanic):
            det.process(xd[cut:], bad)
    es, el = det.process(xd[:0], 1.0)                        # n == 0: OK, nothing produced
    assert tuple(es.shape) == (0,) and tuple(el.shape) == (0, 2)
    s1, l1 = det.process(xd[cut:], 1.0)
    assert torch.equal(torch.cat([s0, s1]), wsym) and torch.equal(torch.cat([l0, l1]), wllr)
    with pytest.raises(ValueError):
        det.process(xd.to(torch.float16), 1.0)


# ------------------------------------------------------------------------- dtypes ----
def test_f16_input(m, torch_cuda):
    """f16 samples are widened exactly: the reference uses the f16 values as float64."""
    torch = torch_cuda
    name = "mfsk4_16"
    _, x, *_ = case(name, 4099, 0.5)
    x16 = x.astype(np.float16)
    E, rsym, rllr, bE, bl, margin = ref_fsk(omega_of(name), 16, x16, 0.25)
    det = _detector(m, name, in_dtype=m.DTYPE_F16)
    parts = [det.process(torch.tensor(c, device="cuda"), 0.25, want_energy=True) for c in (x16[:1001], x16[1001:])]
    sym, llr, en = (torch.cat([p[i] for p in parts]).cpu().numpy() for i in range(3))
    _check(en, E, np.broadcast_to(bE, E.shape), "fsk f16 in energy")
    _check(llr, rllr, np.broadcast_to(bl, rllr.shape), "fsk f16 in llr")
    _check_sym(sym, rsym, margin, bE, "fsk f16 in")


F16_SCALE = 260.0


def test_f16_output_saturates(m, torch_cuda):
    """As test_gpu_diff.py's: in range within the f32 bound + 2^-11 |ref| + 2^-25, exactly +-65504
    where |ref| > 70000, and in between a finite value of at least 0.98 * 65504 with the right sign."""
    torch = torch_cuda
    name = "mfsk4_16"
    _, x, *_ = case(name, 4099, 0.5)
    _, _, ref, _, bl, _ = ref_fsk(omega_of(name), 16, x, F16_SCALE)
    a = np.abs(ref)
    sat, inside = a > 70000, a < 0.99 * 65504
    print(f"fsk f16 out: {int(sat.sum())} saturating, {int(inside.sum())} in range, max |ref| {a.max():.4g}")
    assert sat.sum() >= 8 and inside.sum() >= 8
    assert np.any(ref[sat] > 0) and np.any(ref[sat] < 0)
    _, got = _detector(m, name, llr_dtype=m.DTYPE_F16).process(torch.tensor(x, device="cuda"), F16_SCALE)
    assert got.dtype == torch.float16
    g = got.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(g))
    assert np.array_equal(g[sat], np.sign(ref[sat]) * 65504.0)
    err = np.abs(g - ref)[inside]
    lim = (np.broadcast_to(bl, ref.shape) + 2.0 ** -11 * a + 2.0 ** -25)[inside]
    print(f"fsk f16 out: max err / bound = {np.max(err / lim):.3f}")
    assert np.all(err <= lim)
    mid = ~(sat | inside)
    assert np.all(np.abs(g[mid]) >= 0.98 * 65504) and np.all(np.sign(g[mid]) == np.sign(ref[mid]))


I8_SCALE = 0.5


def test_i8_output(m, torch_cuda):
    """q = rint(clip(ref, -127, 127)): |got - q| <= 1 everywhere, got == q wherever ref lies
    further than the f32 bound from a half-integer (at most 1 % of the elements lie closer)."""
    torch = torch_cuda
    name = "mfsk4_16"
    _, x, *_ = case(name, 4099, 0.5)
    _, _, ref, _, bl, _ = ref_fsk(omega_of(name), 16, x, I8_SCALE)
    q = np.rint(np.clip(ref, -127, 127))
    near = np.abs(ref - (np.floor(ref) + 0.5)) <= bl
    print(f"fsk i8 out: ref in [{ref.min():.4g}, {ref.max():.4g}], {near.mean() * 100:.3f} % near a half-integer")
    assert ref.min() < -127.5 and ref.max() > 127.5 and np.any(np.abs(ref) < 100)
    assert near.mean() <= 0.01
    _, got = _detector(m, name, llr_dtype=m.DTYPE_I8).process(torch.tensor(x, device="cuda"), I8_SCALE)
    assert got.dtype == torch.int8 and tuple(got.shape) == ref.shape
    g = got.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(g - q) <= 1)
    assert np.array_equal(g[~near], q[~near])
    assert g.min() == -127 and g.max() == 127


# --------------------------------------------------------------------------- loopback ----
def _loopback(m, torch, ph, sps, out_mode, bits_np, chunks):
    bps = ph.bits_per_symbol()
    fr = m.Freq(1000, 10000)
    tx = m.DigitalModulator(m.Carrier(fr, 3), ph, sps, None, out_mode=out_mode)
    det = ph.detector(sps, fr if out_mode == m.OUT_IQ_MIXED else None)
    bits = torch.tensor(bits_np, device="cuda")
    syms, llrs = [], []
    a = 0
    for nb, cut in chunks:
        y = tx.process(bits[a:a + nb])
        a += nb
        # `cut`: hand the detector this chunk's samples in two ragged pieces
        for piece in ((y[:cut], y[cut:]) if cut else (y,)):
            s, l = det.process(piece, 1.0)
            syms.append(s)
            llrs.append(l)
    assert a == len(bits_np)
    return torch.cat(syms).cpu().numpy(), torch.cat(llrs).cpu().numpy().reshape(-1, bps)


@pytest.mark.parametrize("mode", ["mixed", "baseband"])
@pytest.mark.parametrize("name", ["mfsk16", "bfsk"])
def test_loopback_recovers_the_bits(m, torch_cuda, name, mode):
    """The detector directly on the TX's device output: every decision is the symbol sent (so the
    first symbol starts at the handle's first sample, modulator.rs:85-100), in one call and with the
    TX and the detector driven in ragged chunks; on the carrier and at baseband."""
    torch = torch_cuda
    mk, sps = {"mfsk16": (lambda: m.MFSK(4, m.Freq(1, 32), 1.0, "default"), 16),
               "bfsk": (lambda: m.BFSK(m.Freq(1, 4), 1.0), 4)}[name]
    out_mode = m.OUT_IQ_MIXED if mode == "mixed" else m.OUT_IQ_BASEBAND
    bps, nsym = mk().bits_per_symbol(), 2048
    bits_np = np.random.RandomState(0xF5C + bps).randint(0, 2, nsym * bps).astype(np.uint8)
    sent = (bits_np.reshape(-1, bps).astype(np.int64) @ (1 << np.arange(bps)[::-1])).astype(np.uint8)
    first = bps * 700 + (1 if bps > 1 else 0)
    second = bps * 5 + (2 if bps > 1 else 0)
    for chunks in ([(nsym * bps, 0)], [(first, sps * 3 + 1), (second, 1), (nsym * bps - first - second, sps * 100 - 1)]):
        sym, llr = _loopback(m, torch, mk(), sps, out_mode, bits_np, chunks)
        assert sym.shape == (nsym,) and llr.shape == (nsym, bps)
        assert np.array_equal(sym, sent)
        assert np.array_equal((llr < 0).astype(np.uint8).reshape(-1), bits_np)
