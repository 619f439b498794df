"""Soft demapper on the GPU: per-bit max-log LLRs against the float64 formula

    d(s)          = (re - lut[s, 0])^2 + (im - lut[s, 1])^2
    llr[k, j]     = scale * (min_{s: bit_j(s)=1} d(s) - min_{s: bit_j(s)=0} d(s)),   j = 0 the MSB

evaluated here in numpy float64 from the same f32 (or f16, widened) inputs and the phasor's
lut() (pinned bit-exact to the oracle by test_capi_host.py).

f32 bound, element-wise: |got - ref| <= 2^-20 * |scale| * max(d0, d1) + 1e-30, with d0, d1 the two
float64 minima. With u = 2^-24: each d carries <= 4u relative error (subtract, square, add), the
difference and the scaling add <= 2u, a different argmin does not matter (the min value is
continuous), so the error is <= 10u * scale * max(d0, d1); 16u leaves margin for either FMA
contraction choice. The bound is derived, not fitted: a miss means the kernel used the expanded
form |r|^2 - 2 r.s + |s|^2 or the wrong levels.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NSYMS = (1, 63, 64, 65, 257, 4099)
APSK_RINGS = [(0, 4, 0.5, float(np.float32(np.pi / 4))), (4, 16, 1.0, float(np.float32(np.pi / 12)))]

# name -> (constructor, amplitude, forced path or None, expected path)
CONSTELLATIONS = {
    "bpsk": (lambda m: m.BPSK(0.3, 2.5), 2.5, None, "general"),
    "qpsk_rot": (lambda m: m.QPSK(0.7, 0.5), 0.5, None, "general"),
    "mpsk8": (lambda m: m.MPSK(3, 0.1, 2.0), 2.0, None, "general"),
    "qam16": (lambda m: m.QAM(4, 0.0, 1.0), 1.0, None, "axis"),
    "apsk16": (lambda m: m.APSK(1.0, 4, [m.Ring(range(a, b), r, ph) for a, b, r, ph in APSK_RINGS]), 1.0,
               None, "general"),
    "qam64_rot": (lambda m: m.QAM(6, 0.2, 3.0), 3.0, None, "general"),
    "qam256": (lambda m: m.QAM(8, 0.0, 1.0), 1.0, None, "axis"),
    "qam256_general": (lambda m: m.QAM(8, 0.0, 1.0), 1.0, "general", "general"),
}
SCALES = {"bpsk": 1.0, "qpsk_rot": 4.0, "mpsk8": 0.75, "qam16": 8.0, "apsk16": 2.5, "qam64_rot": 1.0,
          "qam256": 100.0, "qam256_general": 100.0}       # every one exact in f32


# ------------------------------------------------------------------ inputs and reference ----
@functools.lru_cache(maxsize=None)
def _lut_of(name):
    import __graft_entry__ as graft
    return np.ascontiguousarray(CONSTELLATIONS[name][0](graft.package()).lut(), np.float32)


def _spacing(lut):
    z = lut.astype(np.float64)
    d = np.hypot(z[:, None, 0] - z[None, :, 0], z[:, None, 1] - z[None, :, 1])
    d[np.eye(len(z), dtype=bool)] = np.inf
    return d


def scatter(name, n, seed=0):
    """Seeded Gaussian scatter, sigma = 0.3 x the minimum point spacing, around uniformly drawn points."""
    lut = _lut_of(name)
    rng = np.random.RandomState(0xD3A9 + seed + 7919 * n)
    s = rng.randint(0, len(lut), n)
    sigma = 0.3 * _spacing(lut).min()
    return (lut[s].astype(np.float64) + sigma * rng.standard_normal((n, 2))).astype(np.float32)


def special(name):
    """32 points exactly on the constellation, 32 midpoints between neighbouring points, 8 points
    at 1e3 x the amplitude."""
    lut = _lut_of(name)
    M = len(lut)
    s = (np.arange(32) * 5) % M
    on = lut[s]
    nb = np.argmin(_spacing(lut), axis=1)[s]
    mid = ((lut[s].astype(np.float64) + lut[nb].astype(np.float64)) / 2).astype(np.float32)
    ang = 2 * np.pi * (np.arange(8) + 0.37) / 8
    far = (1e3 * CONSTELLATIONS[name][1] * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([on, mid, far]), np.float32)


def ref_llr(lut, iq, scale):
    """(ref, bound): the float64 LLRs (n, bps) and the f32 bound of the module docstring."""
    z, r = lut.astype(np.float64), np.asarray(iq).astype(np.float64)
    bps = len(lut).bit_length() - 1
    d = (r[:, None, 0] - z[None, :, 0]) ** 2 + (r[:, None, 1] - z[None, :, 1]) ** 2
    s = np.arange(len(lut))
    ref = np.empty((len(r), bps))
    bound = np.empty((len(r), bps))
    for j in range(bps):
        one = ((s >> (bps - 1 - j)) & 1).astype(bool)
        d1, d0 = d[:, one].min(1), d[:, ~one].min(1)
        ref[:, j] = float(scale) * (d1 - d0)
        bound[:, j] = 2.0 ** -20 * abs(float(scale)) * np.maximum(d0, d1) + 1e-30
    return ref, bound


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """(iq f32, ref, bound) of one input set, computed once and shared (treated as read-only)."""
    iq = special(name) if kind == "special" else scatter(name, int(kind))
    ref, bound = ref_llr(_lut_of(name), iq, SCALES[name])
    for a in (iq, ref, bound):
        a.setflags(write=False)
    return iq, ref, bound


def _demapper(m, name, **kw):
    ctor, _, forced, _ = CONSTELLATIONS[name]
    if forced == "general":
        kw["path"] = m.DEMAP_GENERAL
    return m.SoftDemapper(ctor(m), **kw)


def _check_f32(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(np.max(err / bound))
    print(f"{what}: max |got-ref| / bound = {worst:.3f}, max |ref| = {np.abs(ref).max():.4g}")
    assert got.shape == ref.shape
    assert np.all(err <= bound), f"{what}: {int(np.sum(err > bound))} of {err.size} outside the bound (worst {worst:.3f}x)"


def _check_f16(g, ref, bound):
    """f16 output (float64 copy g): finite, exactly +-65504 where |ref| > 70000, the f32 bound +
    2^-11 |ref| + 2^-25 below 0.99 * 65504, and no reference value between the two rules."""
    a = np.abs(ref)
    sat, inside = a > 70000, a < 0.99 * 65504
    assert np.all(sat | inside)
    assert np.all(np.isfinite(g))
    assert np.array_equal(g[sat], np.sign(ref[sat]) * 65504.0)
    err = np.abs(g - ref)[inside]
    lim = (bound + 2.0 ** -11 * a + 2.0 ** -25)[inside]
    print(f"f16 out: max err / bound = {np.max(err / lim):.3f}")
    assert np.all(err <= lim)
    return sat, inside


def _check_i8(g, ref, bound):
    """int8 output (float64 copy g): within 1 of q = rint(clip(ref, -127, 127)) everywhere, equal to
    it wherever ref lies further than the f32 bound from a half-integer (at most 1 % lie closer)."""
    q = np.rint(np.clip(ref, -127, 127))
    near = np.abs(ref - (np.floor(ref) + 0.5)) <= bound
    print(f"i8 out: ref in [{ref.min():.4g}, {ref.max():.4g}], {near.mean() * 100:.3f} % near a half-integer")
    assert ref.min() < -127.5 and ref.max() > 127.5 and np.any(np.abs(ref) < 100)
    assert near.mean() <= 0.01
    assert np.all(np.abs(g - q) <= 1)
    assert np.array_equal(g[~near], q[~near])
    assert g.min() == -127 and g.max() == 127


# ----------------------------------------------------------------------------- parity ----
@pytest.mark.parametrize("kind", [str(n) for n in NSYMS] + ["special"])
@pytest.mark.parametrize("name", list(CONSTELLATIONS))
def test_parity_with_float64(m, torch_cuda, name, kind):
    torch = torch_cuda
    iq, ref, bound = case(name, kind)
    dm = _demapper(m, name)
    got = dm.process(torch.tensor(iq, device="cuda"), SCALES[name])
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape
    _check_f32(got.cpu().numpy(), ref, bound, f"{name}/{kind} ({dm.path})")


@pytest.mark.parametrize("name", list(CONSTELLATIONS))
def test_path_reporting(m, torch_cuda, name):
    assert _demapper(m, name).path == CONSTELLATIONS[name][3]


def test_axis_and_general_agree_on_qam256(m, torch_cuda):
    """Both paths meet the same bound on the same inputs (so they differ by at most twice it)."""
    torch = torch_cuda
    iq, ref, bound = case("qam256", "4099")
    x = torch.tensor(iq, device="cuda")
    ax, ge = m.QAM(8, 0.0, 1.0).demapper(), m.QAM(8, 0.0, 1.0).demapper(path=m.DEMAP_GENERAL)
    assert (ax.path, ge.path) == ("axis", "general")
    a, g = ax.process(x, SCALES["qam256"]).cpu().numpy(), ge.process(x, SCALES["qam256"]).cpu().numpy()
    _check_f32(a, ref, bound, "qam256 axis")
    _check_f32(g, ref, bound, "qam256 general")


def test_qpsk_product_grid_takes_the_axis_path(m, torch_cuda):
    assert m.QPSK(0.0, 1.0).demapper().path == "axis"          # a product grid, bitwise
    assert m.QAM(4, 0.0, 1.0).demapper(path=m.DEMAP_GENERAL).path == "general"
    lut = m.QAM(4, 0.0, 1.0).lut().copy()
    lut[5, 0] = np.nextafter(lut[5, 0], np.float32(2))         # one ulp off the grid: general
    assert m.SoftDemapper(lut).path == "general"


# ------------------------------------------------------------------------- dtypes ----
@pytest.mark.parametrize("path", ["axis", "general"])
def test_f16_input(m, torch_cuda, path):
    """f16 I/Q is widened exactly: the reference uses the f16 values as float64."""
    torch = torch_cuda
    iq16 = np.concatenate([scatter("qam16", 4099, seed=1), special("qam16")]).astype(np.float16)
    ref, bound = ref_llr(_lut_of("qam16"), iq16, 8.0)
    dm = m.QAM(4, 0.0, 1.0).demapper(in_dtype=m.DTYPE_F16, path=m.DEMAP_GENERAL if path == "general" else m.DEMAP_AUTO)
    assert dm.path == path
    got = dm.process(torch.tensor(iq16, device="cuda"), 8.0)
    _check_f32(got.cpu().numpy(), ref, bound, f"qam16 f16 in ({path})")
    with pytest.raises(ValueError):
        dm.process(torch.from_numpy(iq16.astype(np.float32)).cuda(), 8.0)


F16_SCALE = 64.0


def f16_case():
    iq = np.concatenate([scatter("qam16", 4099, seed=2), special("qam16")])
    ref, bound = ref_llr(_lut_of("qam16"), iq, F16_SCALE)
    return iq, ref, bound


def test_f16_output_saturates(m, torch_cuda):
    """Round to nearest, saturating to +-65504, never inf: bound = the f32 bound + 2^-11 |ref| +
    2^-25 (half an ulp of a normal f16, half the subnormal spacing 2^-24) below the f16 range;
    exactly +-65504 where |ref| > 70000. The scale puts reference values on both sides and none
    between 0.99 * 65504 and 70000, where the two rules would meet."""
    torch = torch_cuda
    iq, ref, bound = f16_case()
    a = np.abs(ref)
    sat, inside = a > 70000, a < 0.99 * 65504
    print(f"f16 out: {int(sat.sum())} saturating, {int(inside.sum())} in range, max |ref| {a.max():.4g}")
    assert sat.sum() >= 8 and np.all(sat | inside)
    assert np.any(ref[sat] > 0) and np.any(ref[sat] < 0)
    dm = m.QAM(4, 0.0, 1.0).demapper(out_dtype=m.DTYPE_F16)
    got = dm.process(torch.tensor(iq, device="cuda"), F16_SCALE)
    assert got.dtype == torch.float16
    _check_f16(got.cpu().numpy().astype(np.float64), ref, bound)


I8_SCALE = 256.0


def i8_case():
    iq = scatter("qam16", 4099, seed=3)
    ref, bound = ref_llr(_lut_of("qam16"), iq, I8_SCALE)
    return iq, ref, bound


@pytest.mark.parametrize("path", ["axis", "general"])
def test_i8_output(m, torch_cuda, path):
    """q = rint(clip(ref, -127, 127)): |got - q| <= 1 everywhere, got == q wherever ref lies
    further than the f32 bound from a half-integer (at most 1 % of the elements lie closer)."""
    torch = torch_cuda
    iq, ref, bound = i8_case()
    dm = m.QAM(4, 0.0, 1.0).demapper(out_dtype=m.DTYPE_I8, path=m.DEMAP_GENERAL if path == "general" else m.DEMAP_AUTO)
    got = dm.process(torch.tensor(iq, device="cuda"), I8_SCALE)
    assert got.dtype == torch.int8 and tuple(got.shape) == ref.shape
    _check_i8(got.cpu().numpy().astype(np.float64), ref, bound)


# ------------------------------------------------------------------ chunks and buffers ----
@pytest.mark.parametrize("name", ["qam16", "qam256", "mpsk8"])
@pytest.mark.parametrize("out_dtype", ["f32", "f16", "i8"])
def test_chunks_and_misaligned_output_are_bitwise_identical(m, torch_cuda, name, out_dtype):
    """One call, the same cut 1000 + 3099, and the same into a view that starts one element into
    its buffer (the narrower store path): no stream state, every store width the same bits."""
    torch = torch_cuda
    dt = {"f32": m.DTYPE_F32, "f16": m.DTYPE_F16, "i8": m.DTYPE_I8}[out_dtype]
    tdt = {"f32": torch.float32, "f16": torch.float16, "i8": torch.int8}[out_dtype]
    iq, _, _ = case(name, "4099")
    n, scale = len(iq), {"qam16": 20.0, "qam256": 4000.0, "mpsk8": 20.0}[name]   # i8 outputs mostly non-zero
    x = torch.tensor(iq, device="cuda")
    dm = _demapper(m, name, out_dtype=dt)
    bps = dm.bps
    whole = dm.process(x, scale)
    cut = torch.zeros((n, bps), dtype=tdt, device="cuda")
    dm.process(x[:1000], scale, out=cut[:1000])
    dm.process(x[1000:], scale, out=cut[1000:])
    buf = torch.zeros(n * bps + 1, dtype=tdt, device="cuda")
    view = buf[1:].view(n, bps)
    assert view.data_ptr() % 16 == whole.element_size() and whole.data_ptr() % 16 == 0
    dm.process(x, scale, out=view)
    w = whole.cpu().numpy()
    assert np.count_nonzero(w) > w.size // 2
    assert np.array_equal(w.view(np.uint8), cut.cpu().numpy().view(np.uint8))
    assert np.array_equal(w.view(np.uint8), view.cpu().numpy().view(np.uint8))
    assert buf[0].item() == 0


@pytest.mark.parametrize("out_dtype", ["f32", "i8"])
def test_host_pointers_equal_device(m, torch_cuda, out_dtype):
    torch = torch_cuda
    dt = {"f32": m.DTYPE_F32, "i8": m.DTYPE_I8}[out_dtype]
    iq, _, _ = case("apsk16", "4099")
    dm = _demapper(m, "apsk16", out_dtype=dt)
    dev = dm.process(torch.tensor(iq, device="cuda"), 30.0)
    host = dm.process(np.array(iq), 30.0)
    assert isinstance(host, np.ndarray) and host.shape == (len(iq), 4)
    assert host.dtype == (np.float32 if out_dtype == "f32" else np.int8)
    assert np.array_equal(host.view(np.uint8), dev.cpu().numpy().view(np.uint8))


def test_capacity_and_bad_scale(m, torch_cuda):
    torch = torch_cuda
    iq, _, _ = case("qam16", "257")
    x = torch.tensor(iq, device="cuda")
    dm = _demapper(m, "qam16")
    out = torch.full((257 * 4 - 1,), -7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(m.ModemError) as e:
        dm.process(x, 1.0, out=out)
    assert e.value.status == m.ERR_CAPACITY
    torch.cuda.synchronize()
    assert bool(torch.all(out == -7.0))                      # untouched
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(m.ModemPanic):
            dm.process(x, bad)
    empty = dm.process(x[:0], 1.0)                           # nsym == 0: OK, no launch
    assert tuple(empty.shape) == (0, 4)


# --------------------------------------------------------------------------- loopback ----
def test_loopback_hard_bits(m, torch_cuda):
    """smoke()'s shape, noise-free: 16-QAM, 4 samples/symbol, 129-tap RRC, 2048 symbols. The
    signs of the LLRs are the bits sent and the MSB-first bits of the hard decisions."""
    torch = torch_cuda
    sps, L, nsym = 4, 129, 2048
    taps = m.rrc_taps(L, sps, 0.35)
    qam = m.QAM(4, 0.0, 1.0)
    bits_np = np.random.RandomState(0x5EED).randint(0, 2, nsym * 4).astype(np.uint8)
    w = m.Freq(1, 4).sample_freq()
    tx = m.DigitalModulator(m.Carrier(w), qam, sps, taps)
    y = tx.process(torch.tensor(bits_np, device="cuda"))
    rx = m.DemodulatorRx(m.Carrier(w), taps, decim=sps, decim_offset=L - 1, mix=m.MIX_COMPLEX, slicer=qam.slicer())
    riq, rsym = rx.process(y)
    llr = qam.demapper().process(riq, 1.0).cpu().numpy()
    sym = rsym.cpu().numpy()
    k = len(sym)
    assert k > nsym - L and llr.shape == (k, 4)
    assert not np.any(llr == 0)                              # tie-free: the comparison below is strict
    hard = (llr < 0).astype(np.uint8)
    assert np.array_equal(hard.reshape(-1), bits_np[: k * 4])
    assert np.array_equal(hard, (sym[:, None] >> np.arange(3, -1, -1)) & 1)
