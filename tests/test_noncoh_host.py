"""Noncoherent detectors, host side: the C ABI entry points exist, check their arguments before
they look for a device, report a missing device with a status; the host-side table builders
(modem_phasor_diff_lut, modem_phasor_tones) against numpy; the Python layer's conveniences."""
import ctypes

import numpy as np
import pytest

BAD_DEVICE = 1 << 20      # no machine has this ordinal: NO_DEVICE with or without a GPU
FP = ctypes.POINTER(ctypes.c_float)
SYMBOLS = ("modem_phasor_diff_lut", "modem_phasor_tones", "modem_diff_create", "modem_diff_process",
           "modem_diff_destroy", "modem_fsk_create", "modem_fsk_process", "modem_fsk_destroy")


def _fp(a):
    return None if a is None else a.ctypes.data_as(FP)


def _diff_create(m, lut, bps, prev0, in_dtype, llr_dtype, device, out="handle"):
    h = ctypes.c_void_p(0xDEAD)
    st = m.load_library().modem_diff_create(_fp(lut), bps, _fp(prev0), in_dtype, llr_dtype, device,
                                            None if out is None else ctypes.byref(h))
    return st, h.value


def _fsk_create(m, omega, bps, sps, in_dtype, llr_dtype, device, out="handle"):
    h = ctypes.c_void_p(0xDEAD)
    st = m.load_library().modem_fsk_create(_fp(omega), bps, sps, in_dtype, llr_dtype, device,
                                           None if out is None else ctypes.byref(h))
    return st, h.value


def _ulps(got, want):
    """|got - want| in units of the f32 spacing at `want` (want: float64, exact)."""
    w32 = want.astype(np.float32)
    return np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(np.abs(w32), np.float32(1e-30))).astype(np.float64)


def test_library_exports_the_detectors(m):
    lib = ctypes.CDLL(m.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert m.load_library().modem_abi_version() == 6      # additive: the version stays
    for name in ("DiffDetector", "ToneDetector"):
        assert name in m.__all__ and hasattr(m, name)


def test_null_handles(m):
    L = m.load_library()
    assert L.modem_diff_destroy(None) == m.MODEM_OK          # like free(NULL)
    assert L.modem_fsk_destroy(None) == m.MODEM_OK
    buf = np.zeros(8, np.float32)
    prod = ctypes.c_size_t(77)
    assert L.modem_diff_process(None, buf.ctypes.data, 1, 1.0, None, buf.ctypes.data, 4, None) == m.ERR_INVALID_ARG
    assert L.modem_fsk_process(None, buf.ctypes.data, 1, 1.0, None, buf.ctypes.data, None, 4, ctypes.byref(prod),
                               None) == m.ERR_INVALID_ARG
    assert prod.value == 0


@pytest.mark.parametrize("device", [0, BAD_DEVICE])
def test_diff_invalid_arguments_come_before_the_device_check(m, device):
    lut = np.ascontiguousarray(m.DMPSK(2, 1.0, 0.0, 1.5707964).diff_lut())
    F32, F16, I16, I8 = m.DTYPE_F32, m.DTYPE_F16, m.DTYPE_I16, m.DTYPE_I8
    bad = [
        dict(bps=0), dict(bps=9), dict(bps=255),
        dict(in_dtype=I16), dict(in_dtype=I8), dict(in_dtype=-1), dict(in_dtype=4),
        dict(llr_dtype=I16), dict(llr_dtype=-1), dict(llr_dtype=4),
        dict(lut=None),
    ]
    for kw in bad:
        a = dict(lut=lut, bps=2, in_dtype=F32, llr_dtype=F32)
        a.update(kw)
        st, h = _diff_create(m, a["lut"], a["bps"], None, a["in_dtype"], a["llr_dtype"], device)
        assert st == m.ERR_INVALID_ARG, kw
        assert h is None, kw                                           # *out = NULL
    st, _ = _diff_create(m, lut, 2, None, F32, F32, device, out=None)
    assert st == m.ERR_INVALID_ARG


@pytest.mark.parametrize("device", [0, BAD_DEVICE])
def test_fsk_invalid_arguments_come_before_the_device_check(m, device):
    omega = np.ascontiguousarray(m.MFSK(2, m.Freq(1, 16), 1.0, "increase").tones(0.3))
    F32, F16, I16, I8 = m.DTYPE_F32, m.DTYPE_F16, m.DTYPE_I16, m.DTYPE_I8
    bad = [
        dict(bps=0), dict(bps=9), dict(bps=255), dict(sps=0),
        dict(in_dtype=I16), dict(in_dtype=I8), dict(in_dtype=-1), dict(in_dtype=4),
        dict(llr_dtype=I16), dict(llr_dtype=-1), dict(llr_dtype=4),
        dict(omega=None), dict(omega=np.array([0.1, np.nan, 0.2, 0.3], np.float32)),
    ]
    for kw in bad:
        a = dict(omega=omega, bps=2, sps=8, in_dtype=F32, llr_dtype=F32)
        a.update(kw)
        st, h = _fsk_create(m, a["omega"], a["bps"], a["sps"], a["in_dtype"], a["llr_dtype"], device)
        assert st == m.ERR_INVALID_ARG, kw
        assert h is None, kw
    st, _ = _fsk_create(m, omega, 2, 8, F32, F32, device, out=None)
    assert st == m.ERR_INVALID_ARG
    st, h = _fsk_create(m, omega, 2, 32768, F32, F32, device)          # sps * 2^bps = 131072: the table limit
    assert st == m.ERR_UNSUPPORTED and h is None


def test_valid_create_without_a_device(m):
    lut = np.ascontiguousarray(m.DMPSK(2, 1.0, 0.0, 1.5707964).diff_lut())
    omega = np.ascontiguousarray(m.BFSK(m.Freq(1, 4), 1.0).tones())
    prev0 = np.array([0.5, -0.5], np.float32)
    for llr_dtype in (m.DTYPE_F32, m.DTYPE_F16, m.DTYPE_I8):
        for in_dtype in (m.DTYPE_F32, m.DTYPE_F16):
            for p0 in (None, prev0):
                st, h = _diff_create(m, lut, 2, p0, in_dtype, llr_dtype, BAD_DEVICE)
                assert st == m.ERR_NO_DEVICE and h is None
            st, h = _fsk_create(m, omega, 1, 4, in_dtype, llr_dtype, BAD_DEVICE)
            assert st == m.ERR_NO_DEVICE and h is None
    st, h = _fsk_create(m, omega, 1, 32768, m.DTYPE_F32, m.DTYPE_F32, BAD_DEVICE)   # 65536: within the limit
    assert st == m.ERR_NO_DEVICE and h is None
    for make in (lambda: m.DMPSK(2, 1.0, 0.0, 1.5707964).detector(device=BAD_DEVICE),
                 lambda: m.BFSK(m.Freq(1, 4), 1.0).detector(4, None, device=BAD_DEVICE),
                 lambda: m.DiffDetector(lut, device=BAD_DEVICE),
                 lambda: m.ToneDetector(omega, 4, device=BAD_DEVICE)):
        with pytest.raises(m.ModemError) as e:
            make()
        assert e.value.status == m.ERR_NO_DEVICE and not isinstance(e.value, m.ModemPanic)


# ------------------------------------------------------------------ table builders ----
DMPSK_SHIFTS = [(bps, float(np.float32(2 * np.pi / (1 << bps)))) for bps in (1, 2, 3, 4)] + \
               [(2, 1.5707964), (1, 3.1415927), (3, 0.7), (4, -0.39)]


@pytest.mark.parametrize("bps,shift", DMPSK_SHIFTS)
def test_diff_lut_against_numpy(m, bps, shift):
    lut = m.DMPSK(bps, 1.3, 0.7853982, shift).diff_lut()
    assert lut.shape == (1 << bps, 2) and lut.dtype == np.float32
    a = (np.arange(1 << bps, dtype=np.float32) * np.float32(shift)).astype(np.float64)   # the f32 product
    want = np.stack([np.cos(a), np.sin(a)], 1)
    err = _ulps(lut, want)
    print(f"diff_lut bps {bps} shift {shift}: max {err.max():.3f} ulp")
    assert np.all(err <= 1.0)
    assert lut[0, 0] == 1.0 and lut[0, 1] == 0.0


def _coef(kind, bps):
    s = np.arange(1 << bps)
    return {"default": 2 * s - ((1 << bps) - 1), "increase": 2 * s, "bfsk": s}[kind]


@pytest.mark.parametrize("carrier", [0.0, 0.3, float(np.float32(2 * np.pi * 1000 / 10000))])
@pytest.mark.parametrize("kind,bps,dev", [("default", 4, (1, 32)), ("default", 3, (120, 10000)), ("increase", 2, (1, 16)),
                                          ("increase", 8, (1, 512)), ("default", 1, (50, 10000)), ("bfsk", 1, (1, 4)),
                                          ("bfsk", 1, (200, 10000))])
def test_tones_against_numpy(m, kind, bps, dev, carrier):
    ph = m.BFSK(m.Freq(*dev), 1.0) if kind == "bfsk" else m.MFSK(bps, m.Freq(*dev), 1.0, kind)
    om = ph.tones(carrier)
    assert om.shape == (1 << bps,) and om.dtype == np.float32
    f = np.float64(np.float32(m.Freq(*dev).sample_freq()))
    want = np.float64(np.float32(carrier)) + _coef(kind, bps).astype(np.float64) * f
    err = _ulps(om, want)
    print(f"tones {kind} bps {bps}: max {err.max():.3f} ulp")
    assert np.all(err <= 1.0)
    if carrier == 0.0:
        assert np.array_equal(ph.tones(), om) and np.array_equal(ph.tones(None), om)
    assert np.array_equal(ph.tones(np.float32(carrier)), om)


def test_tones_accept_a_carrier_or_a_freq(m):
    ph = m.MFSK(2, m.Freq(1, 16), 1.0, "increase")
    fr = m.Freq(1000, 10000)
    assert np.array_equal(ph.tones(fr), ph.tones(fr.sample_freq()))
    assert np.array_equal(ph.tones(m.Carrier(fr, 3)), ph.tones(fr.sample_freq()))


def test_builders_reject_other_phasors(m):
    L = m.load_library()
    out = np.zeros(512, np.float32)
    others = [m.BPSK(0.0, 1.0), m.QPSK(0.0, 1.0), m.QAM(4, 0.0, 1.0), m.BASK(1.0), m.MPSK(3, 0.0, 1.0), m.OQPSK(1.0),
              m.DCQPSK(1.0), m.CPFSK(2, m.Rates(100, 1000), 1.0, 1), m.MSK(1.0, 8)]
    for ph in others + [m.MFSK(2, m.Freq(1, 16), 1.0), m.BFSK(m.Freq(1, 4), 1.0)]:
        d = ph._desc()
        assert L.modem_phasor_diff_lut(ctypes.byref(d), _fp(out)) == m.ERR_UNSUPPORTED, type(ph).__name__
    for ph in others + [m.DMPSK(2, 1.0, 0.0, 1.5707964)]:
        d = ph._desc()
        assert L.modem_phasor_tones(ctypes.byref(d), 0.0, _fp(out)) == m.ERR_UNSUPPORTED, type(ph).__name__
    d = m.DMPSK(2, 1.0, 0.0, 1.5707964)._desc()
    assert L.modem_phasor_diff_lut(None, _fp(out)) == m.ERR_INVALID_ARG
    assert L.modem_phasor_diff_lut(ctypes.byref(d), None) == m.ERR_INVALID_ARG
    assert L.modem_phasor_tones(None, 0.0, _fp(out)) == m.ERR_INVALID_ARG
    d.bits_per_symbol = 9
    assert L.modem_phasor_diff_lut(ctypes.byref(d), _fp(out)) == m.ERR_INVALID_ARG


# ------------------------------------------------------------------ Python conveniences ----
def test_phasor_conveniences(m):
    """detector() on a phasor without a noncoherent detector raises what msk.slicer() raises; bad
    arguments panic; a wrong table size panics before the library is asked."""
    msk = m.MSK(1.0, 8)
    with pytest.raises(m.ModemError) as e2:
        msk.slicer()
    for ph in (msk, m.QAM(4, 0.0, 1.0), m.BPSK(0.0, 1.0), m.DCQPSK(1.0), m.CPFSK(2, m.Rates(100, 1000), 1.0, 1)):
        with pytest.raises(m.ModemError) as e:
            ph.detector()
        assert type(e.value) is type(e2.value) and e.value.status == e2.value.status == m.ERR_UNSUPPORTED
        for make in (lambda: m.DiffDetector(ph, device=BAD_DEVICE), lambda: m.ToneDetector(ph, 8, device=BAD_DEVICE)):
            with pytest.raises(m.ModemError) as e:
                make()
            assert e.value.status == m.ERR_UNSUPPORTED
    with pytest.raises(m.ModemError) as e:
        m.DiffDetector(m.BFSK(m.Freq(1, 4), 1.0), device=BAD_DEVICE)
    assert e.value.status == m.ERR_UNSUPPORTED
    with pytest.raises(m.ModemError) as e:
        m.ToneDetector(m.DMPSK(2, 1.0, 0.0, 1.5707964), 4, device=BAD_DEVICE)
    assert e.value.status == m.ERR_UNSUPPORTED
    dq = m.DMPSK(2, 1.0, 0.7853982, 1.5707964)
    with pytest.raises(m.ModemPanic):
        dq.detector(llr_dtype=m.DTYPE_I16, device=BAD_DEVICE)
    with pytest.raises(m.ModemPanic):
        dq.detector(in_dtype=m.DTYPE_I8, device=BAD_DEVICE)
    with pytest.raises(m.ModemPanic):
        m.DiffDetector(np.zeros((3, 2), np.float32), device=BAD_DEVICE)      # not 2^bps rows
    bf = m.BFSK(m.Freq(1, 4), 1.0)
    with pytest.raises(m.ModemPanic):
        bf.detector(0, None, device=BAD_DEVICE)                              # sps < 1
    with pytest.raises(m.ModemPanic):
        bf.detector(4, None, llr_dtype=m.DTYPE_I16, device=BAD_DEVICE)
    with pytest.raises(m.ModemPanic):
        m.ToneDetector(np.zeros(3, np.float32), 4, device=BAD_DEVICE)        # not 2^bps tones
    with pytest.raises(m.ModemError) as e:
        m.ToneDetector(np.zeros(2, np.float32), 65536, device=BAD_DEVICE)    # past the table limit
    assert e.value.status == m.ERR_UNSUPPORTED and not isinstance(e.value, m.ModemPanic)
