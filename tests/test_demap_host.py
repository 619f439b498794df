"""Soft demapper, host side: the C ABI entry points exist, check their arguments before they
look for a device, and report a missing device with a status; the Python layer's conveniences."""
import ctypes

import numpy as np
import pytest

BAD_DEVICE = 1 << 20      # no machine has this ordinal: NO_DEVICE with or without a GPU


def _lut(m, ph):
    return np.ascontiguousarray(ph.lut(), np.float32)


def _create(m, lut, bps, in_dtype, out_dtype, path, device, out="handle"):
    L = m.load_library()
    h = ctypes.c_void_p(0xDEAD)
    st = L.modem_demap_create(None if lut is None else lut.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                              bps, in_dtype, out_dtype, path, device,
                              None if out is None else ctypes.byref(h))
    return st, h.value


def test_library_exports_the_demapper(m):
    lib = ctypes.CDLL(m.lib_path())
    for name in ("modem_demap_create", "modem_demap_process", "modem_demap_path", "modem_demap_destroy"):
        assert hasattr(lib, name), name
    assert m.DTYPE_I8 == 3 and (m.DEMAP_AUTO, m.DEMAP_GENERAL) == (0, 1)
    assert m.load_library().modem_abi_version() == 6      # additive: the version stays


def test_null_handle(m):
    L = m.load_library()
    assert L.modem_demap_path(None) == -1
    assert L.modem_demap_destroy(None) == m.MODEM_OK          # like free(NULL)
    out = np.zeros(4, np.float32)
    assert L.modem_demap_process(None, out.ctypes.data, 1, 1.0, out.ctypes.data, 4, None) == m.ERR_INVALID_ARG
    assert L.modem_demap_process(None, out.ctypes.data, 1, float("nan"), out.ctypes.data, 4, None) == m.ERR_INVALID_ARG


@pytest.mark.parametrize("device", [0, BAD_DEVICE])
def test_invalid_arguments_come_before_the_device_check(m, device):
    lut = _lut(m, m.QAM(4, 0.0, 1.0))
    F32, F16, I16, I8 = m.DTYPE_F32, m.DTYPE_F16, m.DTYPE_I16, m.DTYPE_I8
    bad = [
        dict(bps=0), dict(bps=9), dict(bps=255),                       # bps outside 1..8
        dict(in_dtype=I16), dict(in_dtype=I8), dict(in_dtype=-1), dict(in_dtype=4),
        dict(out_dtype=I16), dict(out_dtype=-1), dict(out_dtype=4),
        dict(path=2), dict(path=-1),
        dict(lut=None),
    ]
    for kw in bad:
        a = dict(lut=lut, bps=4, in_dtype=F32, out_dtype=F32, path=m.DEMAP_AUTO)
        a.update(kw)
        st, h = _create(m, a["lut"], a["bps"], a["in_dtype"], a["out_dtype"], a["path"], device)
        assert st == m.ERR_INVALID_ARG, kw
        assert h is None, kw                                           # *out = NULL
    st, _ = _create(m, lut, 4, F32, F32, m.DEMAP_AUTO, device, out=None)
    assert st == m.ERR_INVALID_ARG


def test_valid_create_without_a_device(m):
    import torch
    lut = _lut(m, m.QAM(4, 0.0, 1.0))
    devices = [BAD_DEVICE, -1] + ([] if torch.cuda.is_available() else [0])
    for device in devices:
        for out_dtype in (m.DTYPE_F32, m.DTYPE_F16, m.DTYPE_I8):
            st, h = _create(m, lut, 4, m.DTYPE_F32, out_dtype, m.DEMAP_AUTO, device)
            assert st == m.ERR_NO_DEVICE, (device, out_dtype)
            assert h is None
    with pytest.raises(m.ModemError) as e:
        m.SoftDemapper(m.QAM(4, 0.0, 1.0), device=BAD_DEVICE)
    assert e.value.status == m.ERR_NO_DEVICE and not isinstance(e.value, m.ModemPanic)


def test_i8_stays_demapper_only(m):
    """MODEM_DTYPE_I8 is additive: the TX and RX entry points keep rejecting it."""
    taps = m.rrc_taps(33, 4, 0.35)
    with pytest.raises(m.ModemPanic):
        m.DigitalModulator(m.Carrier(m.Freq(1, 4)), m.QPSK(0.0, 1.0), 4, taps, dtype=m.DTYPE_I8)
    for kw in (dict(in_dtype=m.DTYPE_I8), dict(out_dtype=m.DTYPE_I8)):
        with pytest.raises(m.ModemPanic):
            m.DemodulatorRx(m.Carrier(m.Freq(1, 4)), taps, decim=4, decim_offset=32, mix=m.MIX_COMPLEX, **kw)


def test_phasor_conveniences(m):
    """_Phasor.demapper(**kw) builds a SoftDemapper from the phasor's table; a sample-dependent
    phasor has none and raises the way its slicer() does."""
    qam = m.QAM(4, 0.0, 1.0)
    with pytest.raises(m.ModemError) as e:
        qam.demapper(out_dtype=m.DTYPE_I8, path=m.DEMAP_GENERAL, device=BAD_DEVICE)
    assert e.value.status == m.ERR_NO_DEVICE              # arguments accepted, then no such device
    with pytest.raises(m.ModemPanic):
        qam.demapper(out_dtype=m.DTYPE_I16, device=BAD_DEVICE)
    with pytest.raises(m.ModemPanic):
        m.SoftDemapper(np.zeros((3, 2), np.float32), device=BAD_DEVICE)   # not 2^bps points
    msk = m.MSK(1.0, 8)
    with pytest.raises(m.ModemError) as e:
        msk.demapper()
    assert e.value.status == m.ERR_UNSUPPORTED
    with pytest.raises(m.ModemError) as e2:
        msk.slicer()
    assert type(e.value) is type(e2.value) and e.value.status == e2.value.status
