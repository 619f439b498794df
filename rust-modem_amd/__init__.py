"""rust_modem_amd — Python mirror of ramtej/rust-modem's modem API over the gfx950 backend.

The product is `lib/libmodem_hip.so` (HIP kernels + the C ABI of include/modem_hip.h); this
module is a thin ctypes layer that keeps the reference crate's names and argument meanings
so callers (and the parity tests) read like the reference:

    reference (src/modem)                          here
    Freq::new(hz, sr).sample_freq()  freq.rs:19-26  Freq(hz, sr).sample_freq()
    Rates::new(br, sr)               rates.rs:12-18 Rates(br, sr).samples_per_symbol
    Carrier::new(freq), .sample      carrier.rs:4-26 Carrier(freq), .sample, .next()
    BPSK/QPSK/QAM/BASK/MPSK/APSK/OQPSK digital/*.rs BPSK(...)... (.i/.q/.bits_per_symbol)
    DigitalModulator::new(&mut c, phasor, src)      DigitalModulator(carrier, phasor, sps, taps)
        modulator.rs:64-101                             .process(bits) -> samples (device)
    FIRFilter::new(&taps).add(x)     fir.rs:3-35    FIRFilter(taps).add(x) / .process(block)
    Demodulator::new(c, sig, lp)     demodulator.rs DemodulatorRx(carrier, taps, ...)
                                                        .process(iq) -> (decimated iq, symbols)

Where the reference panics (assert!, unwrap, index out of range) this layer raises
`ModemPanic`. The HIP library is required: importing works without a GPU (host-only
entry points such as the LUT builders run on the CPU), but every device entry point raises
if the library is missing or no gfx950 device is present — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Optional, Sequence, Tuple

import numpy as np

__all__ = [
    "ModemPanic", "ModemError", "lib_path", "load_library",
    "Freq", "Rates", "Carrier", "Ring",
    "BPSK", "QPSK", "QAM", "BASK", "MPSK", "APSK", "OQPSK",
    "rrc_taps", "DigitalModulator", "DemodulatorRx", "FIRFilter", "prng_bits",
    "MIX_COMPLEX", "MIX_REFERENCE_REAL", "MIX_REFERENCE_REAL_EXACT", "OUT_IQ_MIXED", "OUT_IQ_BASEBAND", "OUT_REAL",
    "TxBatchPlan", "RxBatchPlan", "SLICER_NONE", "SLICER_NEAREST", "SLICER_QAM_AXIS", "DTYPE_F32", "DTYPE_F16", "DTYPE_I16",
    "SoftDemapper", "DTYPE_I8", "DEMAP_AUTO", "DEMAP_GENERAL",
    "DiffDetector", "ToneDetector",
    "Channel", "count_errors",
    "CarrierSync", "SYNC_FLAT",
    "TimingSync",
    "FrameSync",
    "ConvCode", "ViterbiDecoder", "CONV_TAIL",
    "RateMatch", "CRC", "PUNCTURE_2_3", "PUNCTURE_3_4",
]

PI32 = float(np.float32(math.pi))      # std::f32::consts::PI

MODEM_OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_NO_DEVICE, ERR_CAPACITY, ERR_ALLOC = (
    0, -1, -2, -3, -4, -5, -6)
DTYPE_F32, DTYPE_F16, DTYPE_I16 = 0, 1, 2   # I16: real samples, RX input (demodulate)
DTYPE_I8 = 3                                # only as SoftDemapper's out_dtype
DEMAP_AUTO, DEMAP_GENERAL = 0, 1
SYNC_FLAT = 1                               # CarrierSync flags: one phase per block
CONV_TAIL = 1                               # ConvCode flags: K-1 zero bits end each frame in state 0
OUT_IQ_MIXED, OUT_IQ_BASEBAND, OUT_REAL = 0, 1, 2
MIX_COMPLEX, MIX_REFERENCE_REAL, MIX_REFERENCE_REAL_EXACT = 0, 1, 2
SLICER_NONE, SLICER_NEAREST, SLICER_QAM_AXIS = 0, 1, 2
_PH_BPSK, _PH_QPSK, _PH_QAM, _PH_BASK, _PH_MPSK, _PH_APSK, _PH_OQPSK = 1, 2, 3, 4, 5, 6, 7


class ModemError(RuntimeError):
    """A backend failure (HIP error, no device, capacity)."""

    def __init__(self, status: int, what: str = ""):
        self.status = status
        super().__init__(f"{what}: {status_str(status)} ({status})" if what else status_str(status))


class ModemPanic(ModemError):
    """Raised where the reference crate would panic (assert!/unwrap/index)."""


# ------------------------------------------------------------------------- library ----
_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path() -> str:
    # RUST_MODEM_AMD_LIB: an alternative build (profiling ablations, tools/ablate.sh)
    return os.environ.get("RUST_MODEM_AMD_LIB") or os.path.join(_HERE, "lib", "libmodem_hip.so")


class _Ring(ctypes.Structure):
    _fields_ = [("start", ctypes.c_uint8), ("end", ctypes.c_uint8),
                ("radius", ctypes.c_float), ("phase", ctypes.c_float)]


class _PhasorDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("bits_per_symbol", ctypes.c_uint32),
                ("phase", ctypes.c_float), ("amplitude", ctypes.c_float),
                ("nrings", ctypes.c_uint32), ("rings", ctypes.POINTER(_Ring)),
                ("freq", ctypes.c_float), ("samples_per_symbol", ctypes.c_uint32),
                ("shift", ctypes.c_float), ("mfsk_map", ctypes.c_uint32)]


class _SlicerDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("bits_per_symbol", ctypes.c_uint32),
                ("lut", ctypes.POINTER(ctypes.c_float)), ("bits_per_carrier", ctypes.c_uint32),
                ("inv_scale", ctypes.c_float), ("max_symbol", ctypes.c_float)]


class _TxDesc(ctypes.Structure):
    _fields_ = [("bits_per_symbol", ctypes.c_uint32), ("lut", ctypes.POINTER(ctypes.c_float)),
                ("samples_per_symbol", ctypes.c_uint32), ("taps", ctypes.POINTER(ctypes.c_float)),
                ("ntaps", ctypes.c_uint32), ("sample_freq", ctypes.c_float),
                ("s0", ctypes.c_uint64), ("dtype", ctypes.c_int32), ("out_mode", ctypes.c_int32),
                ("q_offset", ctypes.c_uint32), ("phasor", ctypes.POINTER(_PhasorDesc))]


class _RxDesc(ctypes.Structure):
    _fields_ = [("sample_freq", ctypes.c_float), ("s0", ctypes.c_uint64),
                ("taps", ctypes.POINTER(ctypes.c_float)), ("ntaps", ctypes.c_uint32),
                ("decim", ctypes.c_uint32), ("decim_offset", ctypes.c_uint32),
                ("mix", ctypes.c_int32), ("in_dtype", ctypes.c_int32),
                ("out_dtype", ctypes.c_int32), ("slicer", _SlicerDesc),
                ("phase_offset", ctypes.c_float)]


_lib = None
_lib_err: Optional[str] = None


def load_library():
    """Load lib/libmodem_hip.so (raises if it was not built)."""
    global _lib, _lib_err
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        _lib_err = f"{path} not built (run __graft_entry__.build() or `make -C rust-modem_amd`)"
        raise ModemError(ERR_UNSUPPORTED, _lib_err)
    # One HIP runtime per process: torch ships its own libamdhip64 (soname libamdhip64.so.7,
    # loaded by its NEEDED name "libamdhip64.so"). Loading torch first lets our NEEDED
    # libamdhip64.so.7 resolve to that already-loaded runtime, so device pointers and
    # streams from torch are valid here. Without torch, /opt/rocm's runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(path)
    c = ctypes
    vp, sz, u64, u32, f32, st = c.c_void_p, c.c_size_t, c.c_uint64, c.c_uint32, c.c_float, c.c_int
    fp = c.POINTER(c.c_float)
    sig = {
        "modem_status_str": (c.c_char_p, [st]),
        "modem_abi_version": (c.c_int32, []),
        "modem_freq_sample_freq": (f32, [u64, u64]),
        "modem_rates_sps": (st, [u64, u64, c.POINTER(u64)]),
        "modem_pll_lock": (st, [f32, u64, fp, sz, fp]),
        "modem_carrier_phase": (f32, [f32, u64]),
        "modem_carrier_phases": (st, [f32, u64, sz, vp, c.c_int, vp]),
        "modem_phasor_bits": (st, [c.POINTER(_PhasorDesc), c.POINTER(u32)]),
        "modem_phasor_lut": (st, [c.POINTER(_PhasorDesc), fp]),
        "modem_phasor_slicer": (st, [c.POINTER(_PhasorDesc), fp, c.POINTER(_SlicerDesc)]),
        "modem_rrc_taps": (st, [u32, u32, c.c_double, fp]),
        "modem_rrc_taps_offset": (st, [u32, u32, c.c_double, c.c_double, fp]),
        "modem_tx_create": (st, [c.POINTER(_TxDesc), c.c_int, c.POINTER(vp)]),
        "modem_tx_process": (st, [vp, vp, sz, vp, sz, c.POINTER(sz), vp]),
        "modem_tx_flush": (st, [vp, vp, sz, c.POINTER(sz), vp]),
        "modem_tx_process_batch": (st, [c.POINTER(vp), sz, c.POINTER(vp), c.POINTER(sz), c.POINTER(vp),
                                        c.POINTER(sz), c.POINTER(sz), vp]),
        "modem_tx_sample": (u64, [vp]),
        "modem_tx_scan_states": (st, [vp, fp, sz, c.POINTER(sz), vp]),
        "modem_tx_scan_path": (c.c_int, [vp]),
        "modem_tx_destroy": (st, [vp]),
        "modem_rx_create": (st, [c.POINTER(_RxDesc), c.c_int, c.POINTER(vp)]),
        "modem_rx_process": (st, [vp, vp, sz, vp, vp, sz, c.POINTER(sz), vp]),
        "modem_rx_flush": (st, [vp, vp, vp, sz, c.POINTER(sz), vp]),
        "modem_rx_process_batch": (st, [c.POINTER(vp), sz, c.POINTER(vp), c.POINTER(sz), c.POINTER(vp),
                                        c.POINTER(vp), c.POINTER(sz), c.POINTER(sz), vp]),
        "modem_rx_sample": (u64, [vp]),
        "modem_rx_destroy": (st, [vp]),
        "modem_fir_create": (st, [fp, u32, c.c_int, c.POINTER(vp)]),
        "modem_fir_process": (st, [vp, vp, vp, sz, vp]),
        "modem_fir_destroy": (st, [vp]),
        "modem_prng_bits": (st, [u64, vp, sz, c.c_int, vp]),
        "modem_demap_create": (st, [fp, u32, c.c_int32, c.c_int32, c.c_int32, c.c_int, c.POINTER(vp)]),
        "modem_demap_process": (st, [vp, vp, sz, f32, vp, sz, vp]),
        "modem_demap_path": (c.c_int, [vp]),
        "modem_demap_destroy": (st, [vp]),
        "modem_phasor_diff_lut": (st, [c.POINTER(_PhasorDesc), fp]),
        "modem_phasor_tones": (st, [c.POINTER(_PhasorDesc), f32, fp]),
        "modem_diff_create": (st, [fp, u32, fp, c.c_int32, c.c_int32, c.c_int, c.POINTER(vp)]),
        "modem_diff_process": (st, [vp, vp, sz, f32, vp, vp, sz, vp]),
        "modem_diff_destroy": (st, [vp]),
        "modem_fsk_create": (st, [fp, u32, u32, c.c_int32, c.c_int32, c.c_int, c.POINTER(vp)]),
        "modem_fsk_process": (st, [vp, vp, sz, f32, vp, vp, vp, sz, c.POINTER(sz), vp]),
        "modem_fsk_destroy": (st, [vp]),
        "modem_chan_create": (st, [c.c_double, c.c_double, c.c_double, c.c_double, u64, u64, c.c_int32, c.c_int32,
                                   c.c_int, c.POINTER(vp)]),
        "modem_chan_process": (st, [vp, vp, sz, vp, sz, vp]),
        "modem_chan_set_n0": (st, [vp, c.c_double]),
        "modem_chan_nco": (st, [vp, c.POINTER(u64), c.POINTER(u64)]),
        "modem_chan_sample": (u64, [vp]),
        "modem_chan_destroy": (st, [vp]),
        "modem_count_errors": (st, [vp, vp, sz, vp, c.c_int, vp]),
        "modem_sync_create": (st, [u32, u32, c.c_double, c.c_double, c.c_double, u32, c.c_int32, c.c_int32, c.c_int,
                                   c.POINTER(vp)]),
        "modem_sync_process": (st, [vp, vp, sz, vp, sz, vp, vp, sz, c.POINTER(sz), c.POINTER(sz), vp]),
        "modem_sync_flush": (st, [vp, vp, sz, c.POINTER(sz), vp]),
        "modem_sync_symbol": (u64, [vp]),
        "modem_sync_destroy": (st, [vp]),
        "modem_timing_create": (st, [u32, u32, u32, c.c_double, u32, c.c_int32, c.c_int32, c.c_int, c.POINTER(vp)]),
        "modem_timing_process": (st, [vp, vp, sz, vp, sz, vp, vp, sz, c.POINTER(sz), c.POINTER(sz), vp]),
        "modem_timing_flush": (st, [vp, vp, sz, c.POINTER(sz), vp]),
        "modem_timing_sample": (u64, [vp]),
        "modem_timing_destroy": (st, [vp]),
        "modem_frame_create": (st, [fp, u32, u32, c.c_double, c.c_int32, c.c_int, c.POINTER(vp)]),
        "modem_frame_process": (st, [vp, vp, sz, vp, vp, vp, sz, vp, vp]),
        "modem_frame_flush": (st, [vp, vp, vp, vp, sz, vp, vp]),
        "modem_frame_symbol": (u64, [vp]),
        "modem_frame_destroy": (st, [vp]),
        "modem_frame_gather": (st, [vp, sz, u64, vp, vp, vp, sz, u32, u32, u32, c.c_int32, c.c_int32, vp, vp, c.c_int, vp]),
        "modem_conv_encode": (st, [u32, c.POINTER(u32), u32, u32, vp, sz, sz, sz, vp, sz, c.c_int, vp]),
        "modem_viterbi_create": (st, [u32, c.POINTER(u32), u32, u32, c.c_int32, c.c_int, c.POINTER(vp)]),
        "modem_viterbi_process": (st, [vp, vp, sz, sz, sz, f32, vp, vp, sz, vp, vp]),
        "modem_viterbi_destroy": (st, [vp]),
        "modem_rm_kept": (st, [vp, u32, sz, c.POINTER(sz)]),
        "modem_rm_tx": (st, [vp, u32, u32, vp, sz, sz, sz, vp, sz, c.c_int, vp]),
        "modem_rm_rx": (st, [vp, u32, u32, c.c_int32, vp, sz, sz, sz, vp, vp, sz, c.c_int, vp]),
        "modem_crc_attach": (st, [u32, u32, u32, u32, vp, sz, sz, sz, vp, sz, c.c_int, vp]),
        "modem_crc_check": (st, [u32, u32, u32, u32, vp, sz, sz, sz, vp, vp, c.c_int, vp]),
        "modem_chain_create": (st, [vp, vp, vp, sz, vp, sz, vp, vp, sz, c.POINTER(vp)]),
        "modem_chain_run": (st, [vp, c.POINTER(sz), c.POINTER(sz), vp]),
        "modem_chain_fused": (c.c_int, [vp]),
        "modem_chain_destroy": (st, [vp]),
        "modem_chain_batch_create": (st, [c.POINTER(vp), c.POINTER(vp), sz, sz, c.POINTER(vp), c.POINTER(sz),
                                          c.POINTER(vp), c.POINTER(sz), c.POINTER(vp), c.POINTER(vp),
                                          c.POINTER(sz), c.POINTER(vp)]),
        "modem_chain_batch_run": (st, [vp, c.POINTER(sz), c.POINTER(sz), vp]),
        "modem_chain_batch_destroy": (st, [vp]),
    }
    for name, (res, args) in sig.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if name.startswith("modem_chain_"):   # ABI 5; experiment builds of older sources lack it
                continue
            raise
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def status_str(s: int) -> str:
    try:
        return load_library().modem_status_str(s).decode()
    except ModemError:
        return f"status {s}"


def _check(status: int, what: str):
    if status == MODEM_OK:
        return
    if status == ERR_INVALID_ARG:
        raise ModemPanic(status, what)
    raise ModemError(status, what)


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


# --------------------------------------------------------------- timebase (B4) ----
class Freq:
    """freq.rs:3-27 — cycles per second at a sample rate."""

    def __init__(self, hz: int, sr: int):
        self.hz, self.sr = int(hz), int(sr)

    def ang_freq(self) -> float:
        return float(np.float32(2.0) * np.float32(PI32) * np.float32(self.hz))

    def sample_freq(self) -> float:
        return float(load_library().modem_freq_sample_freq(self.hz, self.sr))


class Rates:
    """rates.rs:1-19 — samples_per_symbol = sr / br (integer division)."""

    def __init__(self, br: int, sr: int):
        if br == 0:
            raise ModemPanic(ERR_INVALID_ARG, "Rates::new: attempt to divide by zero")
        self.baud_rate, self.sample_rate = int(br), int(sr)
        self.samples_per_symbol = int(sr) // int(br)


class Carrier:
    """carrier.rs:3-27 — phase(n) = mod_trig(sample_freq * (n as f32)); `sample` is the next n."""

    def __init__(self, freq: Freq, sample: int = 0):
        self.sample_freq = freq.sample_freq() if isinstance(freq, Freq) else float(freq)
        self.sample = int(sample)

    def inner(self, s: int) -> float:
        return float(load_library().modem_carrier_phase(self.sample_freq, int(s)))

    def next(self) -> float:
        s = self.sample
        self.sample += 1
        return self.inner(s)

    def phases(self, s0: int, n: int, device: int = 0, stream=None):
        """inner(s0 .. s0+n-1) on the device (the kernels' phase code path), a CUDA tensor."""
        import torch
        out = torch.empty(int(n), dtype=torch.float32, device=f"cuda:{device}")
        _check(load_library().modem_carrier_phases(self.sample_freq, int(s0), int(n),
                                                   out.data_ptr() if n else None, device,
                                                   _stream_handle(stream, device)), "Carrier.phases")
        return out


# ------------------------------------------------------------ DigitalPhasor (B2) ----
class _Phasor:
    """Memoryless DigitalPhasor (digital/phasor.rs:1-12) as a host-built (I,Q) table."""

    _kind = 0

    def _desc(self) -> _PhasorDesc:
        d = _PhasorDesc()
        d.kind = self._kind
        d.bits_per_symbol = getattr(self, "_bps", 0)
        d.phase = getattr(self, "_phase", 0.0)
        d.amplitude = self.amplitude
        d.nrings = 0
        return d

    def bits_per_symbol(self) -> int:
        b = ctypes.c_uint32()
        _check(load_library().modem_phasor_bits(ctypes.byref(self._desc()), ctypes.byref(b)),
               type(self).__name__)
        return int(b.value)

    def lut(self) -> np.ndarray:
        """(2^bps, 2) float32: row s = (i, q) of the bits of s, MSB first."""
        n = 1 << self.bits_per_symbol()
        out = np.zeros((n, 2), dtype=np.float32)
        _check(load_library().modem_phasor_lut(ctypes.byref(self._desc()), _fptr(out)),
               type(self).__name__)
        return out

    def _index(self, b: Sequence[int]) -> int:
        s = 0
        for v in b:
            s = (s << 1) | (int(v) & 1)   # bytes_to_bits, digital/util.rs:5-11
        return s

    def i(self, s: int, b: Sequence[int]) -> float:
        return float(self.lut()[self._index(b), 0])

    def q(self, s: int, b: Sequence[int]) -> float:
        return float(self.lut()[self._index(b), 1])

    def next(self, s: int, b: Sequence[int]) -> Tuple[float, float]:
        return self.i(s, b), self.q(s, b)

    def slicer(self) -> _SlicerDesc:
        lut = self.lut()
        self._slicer_lut = lut          # keep alive until handed to a handle
        sd = _SlicerDesc()
        _check(load_library().modem_phasor_slicer(ctypes.byref(self._desc()), _fptr(lut),
                                                  ctypes.byref(sd)), "slicer")
        return sd

    def demapper(self, **kw) -> "SoftDemapper":
        """SoftDemapper over this phasor's table (in_dtype, out_dtype, path, device)."""
        return SoftDemapper(self, **kw)

    def synchronizer(self, block: int = 256, **kw) -> "CarrierSync":
        """CarrierSync for this constellation: norm = 1 / rms of the table, M the smallest of 2, 4, 8
        whose M-th power leaves a line, |sum_s (norm lut_s)^M| / sum_s |norm lut_s|^M >= 0.25, and
        ref_phase the argument of that sum (float64). Further keywords go to CarrierSync."""
        power, norm, ref = _sync_params(self.lut(), type(self).__name__)
        return CarrierSync(power, block, norm, ref, **kw)

    def framer(self, uw_symbols, **kw) -> "FrameSync":
        """FrameSync for a unique word of this constellation: u = lut[uw_symbols]; the gather's
        `power` is the M of synchronizer() when the table has a line and 1 otherwise. Further
        keywords go to FrameSync."""
        lut = self.lut()
        idx = np.asarray(uw_symbols, dtype=np.int64).reshape(-1)
        if len(idx) and (idx.min() < 0 or idx.max() >= len(lut)):
            raise ModemPanic(ERR_INVALID_ARG, f"{type(self).__name__}.framer: a symbol outside the table")
        try:
            power = _sync_params(lut, type(self).__name__)[0]
        except ModemPanic:
            power = 1
        f = FrameSync(lut[idx], **kw)
        f.power = power
        return f

    def detector(self, *args, **kw):
        """The noncoherent detector of a phasor that carries state from symbol to symbol (DMPSK,
        MFSK, BFSK); every other phasor is received through slicer() / demapper()."""
        raise ModemError(ERR_UNSUPPORTED, f"{type(self).__name__}: no noncoherent detector")


class BPSK(_Phasor):
    """bpsk.rs:4-32."""
    _kind = _PH_BPSK

    def __init__(self, phase: float, amplitude: float):
        self._phase, self.amplitude = float(phase), float(amplitude)


class QPSK(_Phasor):
    """qpsk.rs:4-36."""
    _kind = _PH_QPSK

    def __init__(self, phase: float, amplitude: float):
        self._phase, self.amplitude = float(phase), float(amplitude)


class QAM(_Phasor):
    """qam.rs:4-61 (natural-binary per axis; I from the MSB half)."""
    _kind = _PH_QAM

    def __init__(self, bits_per_symbol: int, phase: float, amplitude: float):
        if not bits_per_symbol > 1:
            raise ModemPanic(ERR_INVALID_ARG, "QAM::new: assertion failed: bits_per_symbol > 1")
        self._bps, self._phase, self.amplitude = int(bits_per_symbol), float(phase), float(amplitude)


class BASK(_Phasor):
    """bask.rs:3-25."""
    _kind = _PH_BASK

    def __init__(self, a: float):
        self.amplitude = float(a)


class MPSK(_Phasor):
    """mpsk.rs:6-42."""
    _kind = _PH_MPSK

    def __init__(self, bits_per_symbol: int, phase_offset: float, amplitude: float):
        self._bps, self._phase, self.amplitude = int(bits_per_symbol), float(phase_offset), float(amplitude)


class OQPSK(_Phasor):
    """oqpsk.rs:4-26 (the symbol map; pair it with DigitalModulator(even_odd_offset=True),
    the EvenOddOffset source modulate uses, modulate.rs:101-107)."""
    _kind = _PH_OQPSK

    def __init__(self, amplitude: float):
        self.amplitude = float(amplitude)


class Ring:
    """apsk.rs:60-82."""

    def __init__(self, rng: range, radius: float, phase: float):
        if not (0.0 <= radius <= 1.0):
            raise ModemPanic(ERR_INVALID_ARG, "Ring::new: assertion failed: radius in [0, 1]")
        self.range, self.radius, self.phase = rng, float(radius), float(phase)


class APSK(_Phasor):
    """apsk.rs:12-57."""
    _kind = _PH_APSK

    def __init__(self, amplitude: float, bits_per_symbol: int, rings: Sequence[Ring]):
        self.amplitude, self._bps, self.rings = float(amplitude), int(bits_per_symbol), list(rings)
        self.lut()   # verify() (apsk.rs:26) raises ModemPanic on bad rings

    def _desc(self):
        d = super()._desc()
        arr = (_Ring * len(self.rings))()
        for k, r in enumerate(self.rings):
            arr[k].start, arr[k].end = r.range.start, r.range.stop
            arr[k].radius, arr[k].phase = r.radius, r.phase
        self._rings_c = arr
        d.nrings = len(self.rings)
        d.rings = ctypes.cast(arr, ctypes.POINTER(_Ring))
        return d


class _SamplePhasor(_Phasor):
    """A DigitalPhasor whose (i, q) also depend on the symbol count or the sample index: no
    bits-only table; DigitalModulator evaluates it per sample on the GPU (tx_phasor)."""
    sample_dependent = True

    def lut(self) -> np.ndarray:
        raise ModemError(ERR_UNSUPPORTED, f"{type(self).__name__} has no bits-only (I,Q) table")

    def slicer(self):
        raise ModemError(ERR_UNSUPPORTED, f"{type(self).__name__}: no memoryless slicer")

    def demapper(self, **kw):
        raise ModemError(ERR_UNSUPPORTED, f"{type(self).__name__}: no memoryless demapper")

    def framer(self, *args, **kw):
        raise ModemError(ERR_UNSUPPORTED, f"{type(self).__name__}: no symbol table, no frame synchronizer")

    def synchronizer(self, *args, **kw):
        raise ModemError(ERR_UNSUPPORTED, f"{type(self).__name__}: no table to derive a carrier synchronizer from")

    def i(self, s, b):
        raise ModemError(ERR_UNSUPPORTED, "evaluated per sample inside DigitalModulator")

    q = i


class DCQPSK(_SamplePhasor):
    """dcqpsk.rs:8-53 (pi/4-QPSK: the constellation turns by pi/4 at every symbol)."""
    _kind = 8

    def __init__(self, amplitude: float):
        self.amplitude = float(amplitude)


class CPFSK(_SamplePhasor):
    """cpfsk.rs:9-45: CPFSK::new(bits_per_symbol, rates, amplitude, deviation)."""
    _kind = 10

    def __init__(self, bits_per_symbol: int, rates: "Rates", amplitude: float, deviation: int):
        self._bps, self.amplitude = int(bits_per_symbol), float(amplitude)
        self._freq = Freq(int(deviation) * rates.baud_rate // 2, rates.sample_rate).sample_freq()

    def _desc(self):
        d = super()._desc()
        d.freq = self._freq
        return d


class MSK(_SamplePhasor):
    """msk.rs:6-37: MSK::new(amplitude, samples_per_symbol) (modulate pairs it with the
    EvenOddOffset source, modulate.rs:101-107: DigitalModulator(even_odd_offset=True))."""
    _kind = 11

    def __init__(self, amplitude: float, samples_per_symbol: int):
        if int(samples_per_symbol) % 2 != 0:
            raise ModemPanic(ERR_INVALID_ARG, "MSK::new: assertion failed: samples_per_symbol % 2 == 0")
        self.amplitude, self._sps = float(amplitude), int(samples_per_symbol)

    def _desc(self):
        d = super()._desc()
        d.samples_per_symbol = self._sps
        return d


class DMPSK(_SamplePhasor):
    """dmpsk.rs:7-43: DMPSK::new(bits_per_symbol, amplitude, phase, shift); the phase is carried
    in f32 from symbol to symbol (a serial scan on the device)."""
    _kind = 9

    def __init__(self, bits_per_symbol: int, amplitude: float, phase: float, shift: float):
        self._bps, self.amplitude, self._phase, self._shift = int(bits_per_symbol), float(amplitude), \
            float(phase), float(shift)

    def _desc(self):
        d = super()._desc()
        d.shift = self._shift
        return d

    def diff_lut(self) -> np.ndarray:
        """(2^bps, 2) float32: row s = (cos, sin) of the f32 step `s as f32 * shift` (dmpsk.rs:32),
        the table of DiffDetector (modem_phasor_diff_lut)."""
        out = np.zeros((1 << self.bits_per_symbol(), 2), dtype=np.float32)
        _check(load_library().modem_phasor_diff_lut(ctypes.byref(self._desc()), _fptr(out)), "DMPSK.diff_lut")
        return out

    def detector(self, **kw) -> "DiffDetector":
        """DiffDetector for this phasor (prev0, in_dtype, llr_dtype, device); prev0 defaults to the
        point of the initial phase, amplitude * (cos phase, sin phase)."""
        return DiffDetector(self, **kw)


def _tones(self, carrier=None) -> np.ndarray:
    """(2^bps,) float32 tone frequencies in radians per sample (modem_phasor_tones): the carrier's
    sample frequency (a Carrier, a Freq or a float; None = 0, a baseband stream) plus the phasor's
    coef(m) * deviation (mfsk.rs:23-35, bfsk.rs:27-29)."""
    if isinstance(carrier, Freq):
        w = carrier.sample_freq()
    else:
        w = 0.0 if carrier is None else float(getattr(carrier, "sample_freq", carrier))
    out = np.zeros(1 << self.bits_per_symbol(), dtype=np.float32)
    _check(load_library().modem_phasor_tones(ctypes.byref(self._desc()), w, _fptr(out)),
           f"{type(self).__name__}.tones")
    return out


def _tone_detector(self, sps: int, carrier=None, **kw) -> "ToneDetector":
    """ToneDetector over this phasor's tones on `carrier` (in_dtype, llr_dtype, device)."""
    return ToneDetector(self, sps, carrier, **kw)


class MFSK(_SamplePhasor):
    """mfsk.rs:37-85: MFSK::new(bits_per_symbol, deviation: Freq, amplitude, map);
    map "increase" (IncreaseMap, 2s) or "default" (DefaultMap, 2s - max_symbol)."""
    _kind = 12

    def __init__(self, bits_per_symbol: int, deviation: "Freq", amplitude: float, map: str = "default"):
        self._bps, self.amplitude = int(bits_per_symbol), float(amplitude)
        self._freq, self._map = deviation.sample_freq(), 1 if map == "increase" else 0

    def _desc(self):
        d = super()._desc()
        d.freq, d.mfsk_map = self._freq, self._map
        return d

    tones = _tones
    detector = _tone_detector


class BFSK(_SamplePhasor):
    """bfsk.rs:4-56: BFSK::new(deviation: Freq, amplitude)."""
    _kind = 13

    def __init__(self, deviation: "Freq", amplitude: float):
        self.amplitude, self._freq = float(amplitude), deviation.sample_freq()

    def _desc(self):
        d = super()._desc()
        d.freq = self._freq
        return d

    tones = _tones
    detector = _tone_detector


def rrc_taps(ntaps: int, sps: int, beta: float = 0.35, offset: float = 0.0) -> np.ndarray:
    """Root-raised-cosine taps (GLUE: absent from the reference), unit energy, sampled `offset`
    samples late: a TX shaped with them is the nominal TX delayed by `offset` samples."""
    out = np.zeros(int(ntaps), dtype=np.float32)
    _check(load_library().modem_rrc_taps_offset(int(ntaps), int(sps), float(beta), float(offset), _fptr(out)), "rrc_taps")
    return out


# ------------------------------------------------------------- buffers / streams ----
def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


_TORCH = None


def _torch_cuda():
    """torch when it has a GPU, else False (looked up once: is_available() costs ~1 us)."""
    global _TORCH
    if _TORCH is None:
        try:
            import torch
            _TORCH = torch if torch.cuda.is_available() else False
        except ImportError:
            _TORCH = False
    return _TORCH


def _stream_handle(stream, device: Optional[int] = None) -> Optional[int]:
    """The raw HIP stream a call is queued on: `stream` (a torch Stream or a raw handle), else
    torch's current stream of `device` (the handle's GPU; None: the current device), so that
    a handle on another GPU never launches on this device's stream."""
    if stream is not None:
        sdev = getattr(stream, "device_index", None)
        if device is not None and sdev is not None and int(sdev) != int(device):
            raise ValueError(f"stream of cuda:{sdev} given to a handle on cuda:{device}")
        return int(getattr(stream, "cuda_stream", stream))
    t = _torch_cuda()
    if t:
        # the current stream's raw handle (current_stream() builds a Stream object: ~3 us)
        return t._C._cuda_getCurrentRawStream(t._C._cuda_getDevice() if device is None else int(device))
    return None


def _ptr(x) -> int:
    if x is None:
        return 0
    if _is_torch(x):
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return int(x.data_ptr())
    if not x.flags["C_CONTIGUOUS"]:
        raise ValueError("array must be C-contiguous")
    return int(x.ctypes.data)


def _empty_like_input(ref, shape, np_dtype):
    """Allocate an output on the same side (device tensor / host ndarray) as `ref`."""
    if _is_torch(ref):
        import torch
        tdt = {np.float32: torch.float32, np.float16: torch.float16, np.uint8: torch.uint8,
               np.int8: torch.int8}[np_dtype]
        return torch.empty(shape, dtype=tdt, device=ref.device)
    return np.empty(shape, dtype=np_dtype)


def _device_of(x, default: int) -> int:
    if _is_torch(x) and x.is_cuda:
        return int(x.device.index or 0)
    return default


# ------------------------------------------------------------------- TX (B3+B5) ----
class DigitalModulator:
    """DigitalModulator (modulator.rs:64-101) + pulse shaping + IQSample::modulate.

    `process(bits)` takes one byte per bit (values 0/1, data.rs:36) — a CUDA uint8 tensor
    (asynchronous, on the current stream) or a numpy array — and returns the samples of
    every complete symbol: (n, 2) interleaved (i, q) for the IQ modes, (n,) for OUT_REAL.
    `taps=None` keeps the reference's sample-and-hold (bit-compatible with `modulate --iq`).
    `carrier.sample` advances by the samples produced, as the shared `&mut Carrier` does.
    `even_odd_offset=True` is the `EvenOddOffset` source (data.rs:81-123) that `modulate`
    puts under OQPSK (modulate.rs:101-107): Q changes half a symbol after I; it panics
    (ModemPanic) unless the phasor has 2 bits per symbol and samples_per_symbol is even.
    """

    def __init__(self, carrier: Carrier, phasor: _Phasor, samples_per_symbol: int,
                 taps: Optional[np.ndarray] = None, dtype: int = DTYPE_F32,
                 out_mode: int = OUT_IQ_MIXED, device: int = 0, even_odd_offset: bool = False):
        L = load_library()
        self.carrier, self.phasor = carrier, phasor
        self.sps, self.dtype, self.out_mode, self.device = int(samples_per_symbol), dtype, out_mode, device
        self.bps = phasor.bits_per_symbol()
        sample_dep = getattr(phasor, "sample_dependent", False)
        self._lut = None if sample_dep else phasor.lut()
        self.taps = None if taps is None else np.ascontiguousarray(taps, dtype=np.float32)
        d = _TxDesc()
        d.bits_per_symbol = self.bps
        d.lut = _fptr(self._lut) if self._lut is not None else None
        if sample_dep:
            self._pdesc = phasor._desc()
            d.phasor = ctypes.pointer(self._pdesc)
        d.samples_per_symbol = self.sps
        d.taps = _fptr(self.taps) if self.taps is not None else None
        d.ntaps = 0 if self.taps is None else len(self.taps)
        d.sample_freq = carrier.sample_freq
        d.s0 = carrier.sample
        d.dtype, d.out_mode = dtype, out_mode
        d.q_offset = self._q_offset = self.sps // 2 if even_odd_offset else 0
        if even_odd_offset and (self.bps != 2 or self.sps % 2):
            raise ModemPanic(-1, "EvenOddOffset: bits_per_symbol == 2 and an even samples_per_symbol")
        h = ctypes.c_void_p()
        _check(L.modem_tx_create(ctypes.byref(d), device, ctypes.byref(h)), "DigitalModulator")
        self._h = h
        self._ncarry = 0

    def _alloc(self, ref, nsamp: int):
        npd = np.float16 if self.dtype == DTYPE_F16 else np.float32
        shape = (nsamp,) if self.out_mode == OUT_REAL else (nsamp, 2)
        return _empty_like_input(ref, shape, npd)

    def nsamples(self, nbits: int) -> int:
        return ((self._ncarry + nbits) // self.bps) * self.sps

    def process(self, bits, out=None, stream=None):
        n = int(bits.numel() if _is_torch(bits) else bits.size)
        ns = self.nsamples(n)
        if out is None:
            out = self._alloc(bits, ns)
        cap = int(out.shape[0])
        prod = ctypes.c_size_t()
        _check(load_library().modem_tx_process(self._h, _ptr(bits), n, _ptr(out), cap,
                                               ctypes.byref(prod), _stream_handle(stream, self.device)),
               "DigitalModulator.process")
        self._ncarry = (self._ncarry + n) % self.bps
        self.carrier.sample += prod.value        # = modem_tx_sample(h): one sample per output
        return out if prod.value == cap else out[: prod.value]

    @staticmethod
    def process_batch(mods, bits, outs=None, stream=None):
        """`m.process(b)` for every (modulator, bits) pair in order, as one call
        (modem_tx_process_batch): independent channels of one configuration with device
        buffers share one kernel launch per 8 channels. Returns the outputs, as process does."""
        mods, bits = list(mods), list(bits)
        if len(mods) != len(bits) or len(set(map(id, mods))) != len(mods):
            raise ValueError("one bits buffer per distinct modulator")
        n = len(mods)
        nb = [int(b.numel() if _is_torch(b) else b.size) for b in bits]
        if outs is None:
            outs = [m._alloc(b, m.nsamples(k)) for m, b, k in zip(mods, bits, nb)]
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        hs = (vp * n)(*[m._h.value for m in mods])
        prod = (sz * n)()
        _check(load_library().modem_tx_process_batch(
            hs, n, (vp * n)(*[_ptr(b) for b in bits]), (sz * n)(*nb), (vp * n)(*[_ptr(o) for o in outs]),
            (sz * n)(*[int(o.shape[0]) for o in outs]), prod, _stream_handle(stream, mods[0].device)),
            "DigitalModulator.process_batch")
        for m, k in zip(mods, nb):
            m._ncarry = (m._ncarry + k) % m.bps
            m.carrier.sample = int(load_library().modem_tx_sample(m._h))
        return [o[: prod[i]] for i, o in enumerate(outs)]

    def flush(self, like=None, stream=None):
        ntaps = 0 if self.taps is None else len(self.taps)
        tail = ntaps - 1 + self._q_offset if ntaps else 0     # the delayed Q rail drains later
        ns = ((tail + self.sps - 1) // self.sps) * self.sps
        ref = like if like is not None else np.zeros(1, np.uint8)
        out = self._alloc(ref, ns)
        prod = ctypes.c_size_t()
        _check(load_library().modem_tx_flush(self._h, _ptr(out), int(out.shape[0]), ctypes.byref(prod),
                                             _stream_handle(stream, self.device)), "DigitalModulator.flush")
        self.carrier.sample = int(load_library().modem_tx_sample(self._h))
        return out[: prod.value]

    def scan_states(self, stream=None) -> np.ndarray:
        """The (n, 2) float32 per-symbol states that the last process / process_batch call's serial
        scan left on the device (modem_tx_scan_states; DMPSK: (phase, -), MFSK: (cur_coef,
        phase_offset), BFSK: (phase, previous bit)); n = 0 before the first call and after a call
        without a complete symbol. ModemError(ERR_UNSUPPORTED) for every other phasor."""
        L = load_library()
        sh = _stream_handle(stream, self.device)
        n = ctypes.c_size_t()
        status = L.modem_tx_scan_states(self._h, None, 0, ctypes.byref(n), sh)
        if status != ERR_CAPACITY:
            _check(status, "DigitalModulator.scan_states")
        out = np.zeros((n.value, 2), np.float32)
        if n.value:
            _check(L.modem_tx_scan_states(self._h, _fptr(out), n.value, ctypes.byref(n), sh),
                   "DigitalModulator.scan_states")
        return out

    def scan_path(self) -> str:
        """How the last call computed those states (modem_tx_scan_path): "single" (this handle's
        own scan launch), "bank" (process_batch's one launch, a lane per channel) or "none"."""
        return {1: "single", 2: "bank"}.get(load_library().modem_tx_scan_path(self._h), "none")

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.modem_tx_destroy(self._h)
            self._h = None


class TxBatchPlan:
    """A prepared `DigitalModulator.process_batch` over fixed buffers: bits[c] -> outs[c] for
    every channel, the ctypes argument arrays built once, so that each `run()` is one C call
    (modem_tx_process_batch) plus the per-channel bookkeeping. For a channel bank that streams
    through the same device buffers every period."""

    def __init__(self, mods, bits, outs):
        self.mods, self.bits, self.outs = list(mods), list(bits), list(outs)
        n = self.n = len(self.mods)
        if len(self.bits) != n or len(self.outs) != n or len(set(map(id, self.mods))) != n:
            raise ValueError("one bits and one output buffer per distinct modulator")
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        self._nb = [int(b.numel() if _is_torch(b) else b.size) for b in self.bits]
        self._hs = (vp * n)(*[m._h.value for m in self.mods])
        self._bits = (vp * n)(*[_ptr(b) for b in self.bits])
        self._nbits = (sz * n)(*self._nb)
        self._outs = (vp * n)(*[_ptr(o) for o in self.outs])
        self._caps = (sz * n)(*[int(o.shape[0]) for o in self.outs])
        self._prod = (sz * n)()
        self._fn = load_library().modem_tx_process_batch

    def run(self, stream=None):
        """Returns the samples produced per channel (written to outs[c][:produced[c]])."""
        _check(self._fn(self._hs, self.n, self._bits, self._nbits, self._outs, self._caps, self._prod,
                        _stream_handle(stream, self.mods[0].device)), "TxBatchPlan.run")
        L = load_library()
        for m, k in zip(self.mods, self._nb):
            m._ncarry = (m._ncarry + k) % m.bps
            m.carrier.sample = int(L.modem_tx_sample(m._h))
        return list(self._prod)


# ------------------------------------------------------------------- RX (B6+B5) ----
_IN_DTYPE_NAME = {DTYPE_F32: "float32", DTYPE_F16: "float16", DTYPE_I16: "int16"}


def _dtype_name(x) -> str:
    return str(getattr(x, "dtype", "")).replace("torch.", "")


def _check_rx_input(x, in_dtype: int, what: str) -> int:
    """The input must be what the handle was created for — (n, 2) float32 / float16 (i, q) or
    (n,) int16 real samples — else the C side would read n samples of the wrong width.
    Returns n."""
    want = _IN_DTYPE_NAME.get(in_dtype)
    got = _dtype_name(x)
    shape = tuple(int(d) for d in x.shape)
    ok_shape = len(shape) == 1 if in_dtype == DTYPE_I16 else (len(shape) == 2 and shape[1] == 2)
    if got != want or not ok_shape:
        form = "(n,) int16" if in_dtype == DTYPE_I16 else f"(n, 2) {want}"
        raise ValueError(f"{what}: input must be {form} (the handle's in_dtype), got {shape} {got}")
    return shape[0]


class DemodulatorRx:
    """Demodulator (demodulator.rs:7-56) + matched filter + decimation + slicer.

    mix=MIX_REFERENCE_REAL, decim=1 is the reference Demodulator exactly (real input
    x.re, (2*FIR(x cos), 2*FIR(-x sin)) at every sample, PLL offset 0). The loopback
    contract uses MIX_COMPLEX with decim = samples/symbol and decim_offset = ntaps-1.
    """

    def __init__(self, carrier: Carrier, taps: np.ndarray, decim: int = 1, decim_offset: int = 0,
                 mix: int = MIX_REFERENCE_REAL, slicer: Optional[_SlicerDesc] = None,
                 in_dtype: int = DTYPE_F32, out_dtype: int = DTYPE_F32, device: int = 0,
                 phase_offset: float = 0.0):
        L = load_library()
        self.carrier, self.decim, self.out_dtype, self.in_dtype = carrier, int(decim), out_dtype, in_dtype
        self.device = device
        self.taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.decim_offset = int(decim_offset)
        d = _RxDesc()
        d.sample_freq = carrier.sample_freq
        d.s0 = carrier.sample
        d.taps = _fptr(self.taps)
        d.ntaps = len(self.taps)
        d.decim, d.decim_offset, d.mix = self.decim, self.decim_offset, mix
        d.in_dtype, d.out_dtype = in_dtype, out_dtype
        d.phase_offset = float(phase_offset)
        if slicer is not None:
            d.slicer = slicer
        else:
            d.slicer.kind = SLICER_NONE
        self._slicer = slicer
        h = ctypes.c_void_p()
        _check(L.modem_rx_create(ctypes.byref(d), device, ctypes.byref(h)), "Demodulator")
        self._h = h
        self._consumed = 0

    def noutputs(self, n: int) -> int:
        def first(x):
            return 0 if x <= self.decim_offset else (x - self.decim_offset + self.decim - 1) // self.decim
        a, b = first(self._consumed), first(self._consumed + n)
        return max(0, b - a)

    def process(self, iq, want_iq: bool = True, want_sym: bool = True, stream=None,
                out_iq=None, out_sym=None):
        n = _check_rx_input(iq, self.in_dtype, "Demodulator.process")
        nout = self.noutputs(n)
        npd = np.float16 if self.out_dtype == DTYPE_F16 else np.float32
        oiq = out_iq if out_iq is not None else (_empty_like_input(iq, (nout, 2), npd) if want_iq else None)
        osym = out_sym if out_sym is not None else (
            _empty_like_input(iq, (nout,), np.uint8) if (want_sym and self._slicer is not None) else None)
        cap = min(int(oiq.shape[0]) if oiq is not None else nout, int(osym.shape[0]) if osym is not None else nout)
        prod = ctypes.c_size_t()
        _check(load_library().modem_rx_process(self._h, _ptr(iq), n, _ptr(oiq), _ptr(osym), cap,
                                               ctypes.byref(prod), _stream_handle(stream, self.device)),
               "Demodulator.process")
        self._consumed += n
        self.carrier.sample += n                 # = modem_rx_sample(h): one per input sample
        k = prod.value
        return (None if oiq is None else (oiq if int(oiq.shape[0]) == k else oiq[:k])), \
               (None if osym is None else (osym if int(osym.shape[0]) == k else osym[:k]))

    def timing(self, sps: int, block: int = 256, **kw) -> "TimingSync":
        """The symbol timing synchronizer for this RX's output at `sps` samples per symbol, on the
        RX's device and output dtype: the RX must run at sample rate (decim == 1)."""
        if self.decim != 1:
            raise ModemPanic(ERR_INVALID_ARG, "DemodulatorRx.timing: the RX must have decim == 1")
        return TimingSync(sps, block=block, **{"in_dtype": self.out_dtype, "device": self.device, **kw})

    @staticmethod
    def process_batch(rxs, iqs, out_iq=None, out_sym=None, stream=None):
        """`r.process(x)` for every (demodulator, input) pair in order, as one call
        (modem_rx_process_batch): channels of one configuration with device buffers share one
        kernel launch per 8 channels. Returns [(iq, sym), ...] as process does."""
        rxs, iqs = list(rxs), list(iqs)
        if len(rxs) != len(iqs) or len(set(map(id, rxs))) != len(rxs):
            raise ValueError("one input buffer per distinct demodulator")
        n = len(rxs)
        ns = [_check_rx_input(x, r.in_dtype, "Demodulator.process_batch") for r, x in zip(rxs, iqs)]
        nouts = [r.noutputs(k) for r, k in zip(rxs, ns)]
        if out_iq is None:
            out_iq = [_empty_like_input(x, (k, 2), np.float16 if r.out_dtype == DTYPE_F16 else np.float32)
                      for r, x, k in zip(rxs, iqs, nouts)]
        if out_sym is None:
            out_sym = [_empty_like_input(x, (k,), np.uint8) if r._slicer is not None else None
                       for r, x, k in zip(rxs, iqs, nouts)]
        caps = [min(int(a.shape[0]) if a is not None else k, int(b.shape[0]) if b is not None else k)
                for a, b, k in zip(out_iq, out_sym, nouts)]
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        prod = (sz * n)()
        _check(load_library().modem_rx_process_batch(
            (vp * n)(*[r._h.value for r in rxs]), n, (vp * n)(*[_ptr(x) for x in iqs]), (sz * n)(*ns),
            (vp * n)(*[_ptr(a) or None for a in out_iq]), (vp * n)(*[_ptr(b) or None for b in out_sym]),
            (sz * n)(*caps), prod, _stream_handle(stream, rxs[0].device)), "Demodulator.process_batch")
        res = []
        for i, (r, k) in enumerate(zip(rxs, ns)):
            r._consumed += k
            r.carrier.sample = int(load_library().modem_rx_sample(r._h))
            a, b = out_iq[i], out_sym[i]
            res.append((None if a is None else a[: prod[i]], None if b is None else b[: prod[i]]))
        return res

    def flush(self, like=None, stream=None):
        n = len(self.taps) - 1
        nout = self.noutputs(n)
        ref = like if like is not None else np.zeros(1, np.float32)
        npd = np.float16 if self.out_dtype == DTYPE_F16 else np.float32
        oiq = _empty_like_input(ref, (nout, 2), npd)
        osym = _empty_like_input(ref, (nout,), np.uint8) if self._slicer is not None else None
        prod = ctypes.c_size_t()
        _check(load_library().modem_rx_flush(self._h, _ptr(oiq), _ptr(osym), nout, ctypes.byref(prod),
                                             _stream_handle(stream, self.device)), "Demodulator.flush")
        self._consumed += n
        self.carrier.sample = int(load_library().modem_rx_sample(self._h))
        return oiq[: prod.value], (None if osym is None else osym[: prod.value])

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.modem_rx_destroy(self._h)
            self._h = None


# --------------------------------------------------------------------- FIR (B5) ----
LOCK_SAMPLES = 64   # demodulator.rs:5


class Demodulator:
    """Demodulator (demodulator.rs:7-56) with its PLL lock, as the `demodulate` binary drives it
    (demodulate.rs:29-43): `lock_phase(sig)` runs PLL::handle (pll.rs:16-22) over the first 64
    complex samples (host, modem_pll_lock: 64 serial steps of control logic), then `process`
    gives (2*FIR(x.re*cos), 2*FIR(-x.re*sin)) at every further sample on the GPU with the locked
    offset (`phase = carrier.next() + pll.phase_offset`, demodulator.rs:50) — by default with
    MIX_REFERENCE_REAL_EXACT, bit-identical to the reference (exact=False: the fast real mix,
    within 1e-5). `sig`: (n, 2) float32 (re, im) — a CUDA tensor or a numpy array — or, for
    `process`, (n,) int16 real samples."""

    def __init__(self, carrier: Carrier, lowpass: np.ndarray, device: int = 0, exact: bool = True):
        self.carrier, self.lowpass, self.device = carrier, np.ascontiguousarray(lowpass, np.float32), device
        self.exact = exact
        self.phase_offset = 0.0
        self._rx = None

    def lock_phase(self, sig):
        """Consume the first 64 samples of `sig` (demodulator.rs:32-36); returns the rest."""
        head = sig[:LOCK_SAMPLES]
        if int(head.shape[0]) < LOCK_SAMPLES:
            raise ModemPanic(ERR_INVALID_ARG, "lock_phase: called `Option::unwrap()` on a `None` value")
        h = np.ascontiguousarray(head.detach().cpu().numpy() if _is_torch(head) else head, np.float32)
        off = (ctypes.c_float * 1)(self.phase_offset)
        _check(load_library().modem_pll_lock(self.carrier.sample_freq, self.carrier.sample, _fptr(h),
                                             LOCK_SAMPLES, off), "Demodulator.lock_phase")
        self.phase_offset = float(off[0])
        self.carrier.sample += LOCK_SAMPLES
        return sig[LOCK_SAMPLES:]

    def process(self, sig, stream=None):
        """(n, 2) float32 (i, q), one per input sample (Iterator::next, demodulator.rs:44-56)."""
        if self._rx is None:
            i16 = _dtype_name(sig) == "int16"
            if i16 and not self.exact:
                raise ValueError("Demodulator.process: int16 input needs exact=True "
                                 "(MIX_REFERENCE_REAL_EXACT reads i16 samples; the fast real mix does not)")
            self._rx = DemodulatorRx(self.carrier, self.lowpass, decim=1, decim_offset=0,
                                     mix=MIX_REFERENCE_REAL_EXACT if self.exact else MIX_REFERENCE_REAL,
                                     in_dtype=DTYPE_I16 if i16 else DTYPE_F32, device=self.device,
                                     phase_offset=self.phase_offset)
        iq, _ = self._rx.process(sig, want_sym=False, stream=stream)
        return iq


class FIRFilter:
    """FIRFilter (fir.rs:3-35): causal FIR, zero initial history, one output per input."""

    def __init__(self, coefs, device: int = 0):
        self.device = device
        self.coefs = np.ascontiguousarray(coefs, dtype=np.float32)
        if len(self.coefs) == 0:
            raise ModemPanic(ERR_INVALID_ARG, "FIRFilter: attempt to calculate the remainder with a divisor of zero")
        h = ctypes.c_void_p()
        _check(load_library().modem_fir_create(_fptr(self.coefs), len(self.coefs), device, ctypes.byref(h)),
               "FIRFilter")
        self._h = h

    def process(self, x, stream=None):
        n = int(x.shape[0])
        y = _empty_like_input(x, (n,), np.float32)
        _check(load_library().modem_fir_process(self._h, _ptr(x), _ptr(y), n, _stream_handle(stream, self.device)),
               "FIRFilter.process")
        return y

    def add(self, sample: float) -> float:
        return float(self.process(np.array([sample], dtype=np.float32))[0])

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.modem_fir_destroy(self._h)
            self._h = None


# ------------------------------------------------------------------ soft demapper ----
_LLR_DTYPE = {DTYPE_F32: np.float32, DTYPE_F16: np.float16, DTYPE_I8: np.int8}


class SoftDemapper:
    """Per-bit max-log LLRs of received points (GLUE: the reference ends at hard symbols).

    llr[k, j] = scale * (min_{s: bit_j(s)=1} |r_k - lut[s]|^2 - min_{s: bit_j(s)=0} |r_k - lut[s]|^2),
    j = 0 the MSB (the order of the TX's one-byte-per-bit input); positive = "bit 0 more likely",
    the hard bit is llr < 0. `phasor_or_lut`: a memoryless phasor or its (2^bps, 2) float32 table.
    `process(iq, scale)` takes the (n, 2) I/Q that `DemodulatorRx.process` returns — a CUDA
    tensor (asynchronous, on the current stream) or a numpy array — and returns (n, bps) of
    out_dtype (float32, float16 saturating at +-65504, or int8 = rint(clamp(llr, -127, 127)))
    on the same side. Pass scale = 1/N0, times a quantiser gain for int8."""

    def __init__(self, phasor_or_lut, in_dtype: int = DTYPE_F32, out_dtype: int = DTYPE_F32,
                 path: int = DEMAP_AUTO, device: int = 0):
        lut = phasor_or_lut.lut() if isinstance(phasor_or_lut, _Phasor) else phasor_or_lut
        self.lut = np.ascontiguousarray(lut, dtype=np.float32).reshape(-1, 2)
        n = self.lut.shape[0]
        bps = n.bit_length() - 1
        if n < 2 or n != 1 << bps:
            raise ModemPanic(ERR_INVALID_ARG, f"SoftDemapper: a table of {n} points is not 2^bps")
        self.bps, self.in_dtype, self.out_dtype, self.device = bps, in_dtype, out_dtype, device
        h = ctypes.c_void_p()
        _check(load_library().modem_demap_create(_fptr(self.lut), bps, in_dtype, out_dtype, path, device,
                                                 ctypes.byref(h)), "SoftDemapper")
        self._h = h

    @property
    def path(self) -> str:
        return "axis" if load_library().modem_demap_path(self._h) == 1 else "general"

    def process(self, iq, scale: float, out=None, stream=None):
        n = _check_rx_input(iq, self.in_dtype, "SoftDemapper.process")
        llr = out if out is not None else _empty_like_input(iq, (n, self.bps), _LLR_DTYPE[self.out_dtype])
        if _dtype_name(llr) != np.dtype(_LLR_DTYPE[self.out_dtype]).name:
            raise ValueError(f"SoftDemapper.process: out must be {np.dtype(_LLR_DTYPE[self.out_dtype]).name} "
                             f"(the handle's out_dtype), got {_dtype_name(llr)}")
        cap = 1
        for d in llr.shape:
            cap *= int(d)
        _check(load_library().modem_demap_process(self._h, _ptr(iq), n, float(scale), _ptr(llr), cap,
                                                  _stream_handle(stream, self.device)), "SoftDemapper.process")
        return llr

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.modem_demap_destroy(self._h)
            self._h = None


# ----------------------------------------------------------- noncoherent detectors ----
def _check_out(x, np_dtype, what: str):
    if _dtype_name(x) != np.dtype(np_dtype).name:
        raise ValueError(f"{what} must be {np.dtype(np_dtype).name}, got {_dtype_name(x)}")
    n = 1
    for d in x.shape:
        n *= int(d)
    return n


class DiffDetector:
    """Differential detector (GLUE: the reference has none) for DMPSK (dmpsk.rs:29-43), at symbol
    rate on the (n, 2) I/Q that `DemodulatorRx.process` returns.

    z[k] = r[k] * conj(r[k-1]), c(s) = z.re * lut[s, 0] + z.im * lut[s, 1]; sym[k] = argmax_s c(s)
    (lowest index on ties); llr[k, j] = scale * (max_{bit_j(s)=0} c(s) - max_{bit_j(s)=1} c(s)),
    j = 0 the MSB, positive = "bit 0 more likely". r[-1] is the last point of the previous call,
    `prev0` before the first. `phasor_or_table`: a DMPSK phasor or a (2^bps, 2) float32 table.
    `process(iq, scale)` returns (sym, llr): (n,) uint8 and (n, bps) of llr_dtype, on the side of
    the input (CUDA tensors, asynchronous on the current stream, or numpy arrays)."""

    def __init__(self, phasor_or_table, prev0=None, in_dtype: int = DTYPE_F32, llr_dtype: int = DTYPE_F32,
                 device: int = 0):
        if isinstance(phasor_or_table, _Phasor):
            ph = phasor_or_table
            if not isinstance(ph, DMPSK):
                raise ModemError(ERR_UNSUPPORTED, f"{type(ph).__name__}: no differential detector")
            lut = ph.diff_lut()
            if prev0 is None:
                prev0 = (ph.amplitude * math.cos(ph._phase), ph.amplitude * math.sin(ph._phase))
        else:
            lut = phasor_or_table
        self.lut = np.ascontiguousarray(lut, dtype=np.float32).reshape(-1, 2)
        n = self.lut.shape[0]
        bps = n.bit_length() - 1
        if n < 2 or n != 1 << bps:
            raise ModemPanic(ERR_INVALID_ARG, f"DiffDetector: a table of {n} rows is not 2^bps")
        self.bps, self.in_dtype, self.llr_dtype, self.device = bps, in_dtype, llr_dtype, device
        self.prev0 = None if prev0 is None else np.ascontiguousarray(prev0, dtype=np.float32).reshape(2)
        h = ctypes.c_void_p()
        _check(load_library().modem_diff_create(_fptr(self.lut), bps, None if self.prev0 is None else _fptr(self.prev0),
                                                in_dtype, llr_dtype, device, ctypes.byref(h)), "DiffDetector")
        self._h = h

    def process(self, iq, scale: float = 1.0, out_sym=None, out_llr=None, stream=None):
        n = _check_rx_input(iq, self.in_dtype, "DiffDetector.process")
        sym = out_sym if out_sym is not None else _empty_like_input(iq, (n,), np.uint8)
        llr = out_llr if out_llr is not None else _empty_like_input(iq, (n, self.bps), _LLR_DTYPE[self.llr_dtype])
        cap = min(_check_out(sym, np.uint8, "DiffDetector.process: out_sym"),
                  _check_out(llr, _LLR_DTYPE[self.llr_dtype], "DiffDetector.process: out_llr") // self.bps)
        _check(load_library().modem_diff_process(self._h, _ptr(iq), n, float(scale), _ptr(sym), _ptr(llr), cap,
                                                 _stream_handle(stream, self.device)), "DiffDetector.process")
        return sym, llr

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.modem_diff_destroy(self._h)
            self._h = None


class ToneDetector:
    """Tone-bank energy detector (GLUE: the reference has none) for MFSK (mfsk.rs:60-75) and BFSK
    (bfsk.rs:23-55), at sample rate directly on the (n, 2) complex samples of `DigitalModulator`.

    Symbol k covers the samples k*sps .. k*sps+sps-1 from the detector's first input sample:
    E[k, m] = |sum_i x[k*sps+i] * e^{-j omega[m] i}|^2; sym[k] = argmax_m E[k, m] (lowest index on
    ties); llr[k, j] = scale * (max_{bit_j(m)=0} E - max_{bit_j(m)=1} E), j = 0 the MSB.
    `omega_or_phasor`: an MFSK / BFSK phasor (its tones on `carrier`: a Carrier, a Freq, a float, or
    None for a baseband stream) or (2^bps,) float32 tone frequencies in radians per sample.
    `process(x, scale)` returns (sym, llr) for the floor((carried + n) / sps) symbols the call
    completes — the < sps samples left over carry into the next call — on the side of the input;
    `want_energy=True` (or `out_energy`) adds the (k, 2^bps) float32 energies as a third value."""

    def __init__(self, omega_or_phasor, sps: int, carrier=None, in_dtype: int = DTYPE_F32,
                 llr_dtype: int = DTYPE_F32, device: int = 0):
        if isinstance(omega_or_phasor, _Phasor):
            ph = omega_or_phasor
            if not isinstance(ph, (MFSK, BFSK)):
                raise ModemError(ERR_UNSUPPORTED, f"{type(ph).__name__}: no tone-bank detector")
            omega = ph.tones(carrier)
        else:
            omega = omega_or_phasor
        self.omega = np.ascontiguousarray(omega, dtype=np.float32).reshape(-1)
        n = self.omega.shape[0]
        bps = n.bit_length() - 1
        if n < 2 or n != 1 << bps:
            raise ModemPanic(ERR_INVALID_ARG, f"ToneDetector: {n} tones are not 2^bps")
        self.bps, self.sps, self.in_dtype, self.llr_dtype, self.device = bps, int(sps), in_dtype, llr_dtype, device
        if self.sps < 1:
            raise ModemPanic(ERR_INVALID_ARG, "ToneDetector: samples per symbol < 1")
        h = ctypes.c_void_p()
        _check(load_library().modem_fsk_create(_fptr(self.omega), bps, self.sps, in_dtype, llr_dtype, device,
                                               ctypes.byref(h)), "ToneDetector")
        self._h = h
        self._ncarry = 0

    def nsymbols(self, n: int) -> int:
        return (self._ncarry + int(n)) // self.sps

    def process(self, x, scale: float = 1.0, out_sym=None, out_llr=None, out_energy=None, want_energy: bool = False,
                stream=None):
        n = _check_rx_input(x, self.in_dtype, "ToneDetector.process")
        k = self.nsymbols(n)
        sym = out_sym if out_sym is not None else _empty_like_input(x, (k,), np.uint8)
        llr = out_llr if out_llr is not None else _empty_like_input(x, (k, self.bps), _LLR_DTYPE[self.llr_dtype])
        en = out_energy if out_energy is not None else (
            _empty_like_input(x, (k, 1 << self.bps), np.float32) if want_energy else None)
        cap = min(_check_out(sym, np.uint8, "ToneDetector.process: out_sym"),
                  _check_out(llr, _LLR_DTYPE[self.llr_dtype], "ToneDetector.process: out_llr") // self.bps)
        if en is not None:
            cap = min(cap, _check_out(en, np.float32, "ToneDetector.process: out_energy") >> self.bps)
        prod = ctypes.c_size_t()
        _check(load_library().modem_fsk_process(self._h, _ptr(x), n, float(scale), _ptr(sym), _ptr(llr), _ptr(en),
                                                cap, ctypes.byref(prod), _stream_handle(stream, self.device)),
               "ToneDetector.process")
        self._ncarry = (self._ncarry + n) % self.sps
        p = prod.value
        res = tuple(a if int(a.shape[0]) == p else a[:p] for a in ((sym, llr) if en is None else (sym, llr, en)))
        return res

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.modem_fsk_destroy(self._h)
            self._h = None


class RxBatchPlan:
    """A prepared `DemodulatorRx.process_batch` over fixed buffers (iqs[c] -> out_iq[c],
    out_sym[c]; either output may be None): each `run()` is one modem_rx_process_batch call."""

    def __init__(self, rxs, iqs, out_iq, out_sym):
        self.rxs, self.iqs = list(rxs), list(iqs)
        n = self.n = len(self.rxs)
        out_iq, out_sym = list(out_iq), list(out_sym)
        if len(self.iqs) != n or len(out_iq) != n or len(out_sym) != n or len(set(map(id, self.rxs))) != n:
            raise ValueError("one input and one output set per distinct demodulator")
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        self._ns = [_check_rx_input(x, r.in_dtype, "RxBatchPlan") for r, x in zip(self.rxs, self.iqs)]
        caps = [min(int(a.shape[0]) if a is not None else 1 << 62, int(b.shape[0]) if b is not None else 1 << 62)
                for a, b in zip(out_iq, out_sym)]
        self._hs = (vp * n)(*[r._h.value for r in self.rxs])
        self._ins = (vp * n)(*[_ptr(x) for x in self.iqs])
        self._nsa = (sz * n)(*self._ns)
        self._oiq = (vp * n)(*[_ptr(a) or None for a in out_iq])
        self._osym = (vp * n)(*[_ptr(b) or None for b in out_sym])
        self._caps = (sz * n)(*caps)
        self._prod = (sz * n)()
        self._fn = load_library().modem_rx_process_batch

    def run(self, stream=None):
        """Returns the kept instants produced per channel."""
        _check(self._fn(self._hs, self.n, self._ins, self._nsa, self._oiq, self._osym, self._caps, self._prod,
                        _stream_handle(stream, self.rxs[0].device)), "RxBatchPlan.run")
        L = load_library()
        for r, k in zip(self.rxs, self._ns):
            r._consumed += k
            r.carrier.sample = int(L.modem_rx_sample(r._h))
        return list(self._prod)


class ChainPlan:
    """One period of the sample-buffer loop as one C call (modem_chain_*): `run()` equals
    `tx.process(bits, out=samples)` followed by `rx.process(samples, out_iq=out_iq,
    out_sym=out_sym)` — the DigitalModulator's samples of the bit buffer (modulator.rs:85-100),
    then the Demodulator over them (demodulator.rs:44-56) — with the device buffers checked once
    here instead of on every call. Both handles' Python-side state (carried bits, carrier
    sample, consumed samples) advances as those calls would advance it."""

    def __init__(self, tx: "DigitalModulator", rx: "DemodulatorRx", bits, samples, out_iq=None, out_sym=None):
        self.tx, self.rx = tx, rx
        self.bits, self.samples, self.out_iq, self.out_sym = bits, samples, out_iq, out_sym
        if tx.dtype != rx.in_dtype or tx.out_mode == OUT_REAL:
            raise ValueError("ChainPlan: the RX must read the TX's interleaved samples (one dtype)")
        # the C side sizes every buffer from its first dimension: a buffer of the wrong width
        # would be written past its end on the device
        _check_rx_input(samples, tx.dtype, "ChainPlan samples")
        want_out = _IN_DTYPE_NAME[rx.out_dtype]
        if out_iq is not None and (len(out_iq.shape) != 2 or int(out_iq.shape[1]) != 2
                                   or _dtype_name(out_iq) != want_out):
            raise ValueError(f"ChainPlan: out_iq must be (k, 2) {want_out} (the RX's out_dtype), "
                             f"got {tuple(out_iq.shape)} {_dtype_name(out_iq)}")
        if out_sym is not None and (len(out_sym.shape) != 1 or _dtype_name(out_sym) != "uint8"):
            raise ValueError(f"ChainPlan: out_sym must be (k,) uint8, got {tuple(out_sym.shape)} {_dtype_name(out_sym)}")
        self._nbits = int(bits.numel() if _is_torch(bits) else bits.size)
        caps = [int(x.shape[0]) for x in (out_iq, out_sym) if x is not None]
        h = ctypes.c_void_p()
        _check(load_library().modem_chain_create(tx._h, rx._h, _ptr(bits), self._nbits, _ptr(samples),
                                                 int(samples.shape[0]), _ptr(out_iq) or None, _ptr(out_sym) or None,
                                                 min(caps) if caps else 1 << 62, ctypes.byref(h)), "ChainPlan")
        self._h = h
        self._n, self._k = ctypes.c_size_t(), ctypes.c_size_t()
        self._pn, self._pk = ctypes.byref(self._n), ctypes.byref(self._k)
        self._fn = load_library().modem_chain_run

    def run(self, stream=None):
        """Returns (samples produced, kept instants produced)."""
        _check(self._fn(self._h, self._pn, self._pk, _stream_handle(stream, self.tx.device)), "ChainPlan.run")
        n = self._n.value
        tx, rx = self.tx, self.rx
        tx._ncarry = (tx._ncarry + self._nbits) % tx.bps
        tx.carrier.sample += n
        rx._consumed += n
        rx.carrier.sample += n
        return n, self._k.value

    @property
    def fused(self) -> int:
        """1 or 2: the last run() was one launch (TX and RX of the period fused; 2: with the
        samples handed over in LDS), 0: two launches, -1: no run yet."""
        return int(load_library().modem_chain_fused(self._h))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.modem_chain_destroy(self._h)
            self._h = None


class ChainBatchPlan:
    """One period of a bank of independent channels as one C call (modem_chain_batch_*): `run()`
    equals `ChainPlan(tx[i], rx[i], bits[i], samples[i], out_iq[i], out_sym[i]).run()` for every
    channel i (the DigitalModulator's samples of each channel's bits, modulator.rs:85-100, then
    that channel's Demodulator over them, demodulator.rs:44-56), run as one TX launch and then one
    RX launch per `group` consecutive channels, with the handles and buffers checked once here.
    Every handle's Python-side state advances as those calls would advance it. Raises ModemError
    (MODEM_ERR_UNSUPPORTED) when the handles do not share one matrix-core configuration per side."""

    def __init__(self, txs, rxs, bits, samples, out_iq, out_sym, group: int = 8):
        self.txs, self.rxs = list(txs), list(rxs)
        self.bits, self.samples, self.out_iq, self.out_sym = list(bits), list(samples), list(out_iq), list(out_sym)
        n = self.n = len(self.txs)
        if not (len(self.rxs) == len(self.bits) == len(self.samples) == len(self.out_iq) == len(self.out_sym) == n):
            raise ValueError("ChainBatchPlan: one modulator, demodulator and buffer set per channel")
        for tx, rx, y, oiq, osym in zip(self.txs, self.rxs, self.samples, self.out_iq, self.out_sym):
            if tx.dtype != rx.in_dtype or tx.out_mode == OUT_REAL:
                raise ValueError("ChainBatchPlan: each RX must read its TX's interleaved samples (one dtype)")
            _check_rx_input(y, tx.dtype, "ChainBatchPlan samples")
            want_out = _IN_DTYPE_NAME[rx.out_dtype]
            if len(oiq.shape) != 2 or int(oiq.shape[1]) != 2 or _dtype_name(oiq) != want_out:
                raise ValueError(f"ChainBatchPlan: out_iq must be (k, 2) {want_out}, got {tuple(oiq.shape)} {_dtype_name(oiq)}")
            if len(osym.shape) != 1 or _dtype_name(osym) != "uint8":
                raise ValueError(f"ChainBatchPlan: out_sym must be (k,) uint8, got {tuple(osym.shape)} {_dtype_name(osym)}")
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        self._nb = [int(b.numel() if _is_torch(b) else b.size) for b in self.bits]
        txh = (vp * n)(*[t._h.value for t in self.txs])
        rxh = (vp * n)(*[r._h.value for r in self.rxs])
        outc = (sz * n)(*[min(int(a.shape[0]), int(b.shape[0])) for a, b in zip(self.out_iq, self.out_sym)])
        h = ctypes.c_void_p()
        _check(load_library().modem_chain_batch_create(
            txh, rxh, n, int(group), (vp * n)(*[_ptr(b) for b in self.bits]), (sz * n)(*self._nb),
            (vp * n)(*[_ptr(y) for y in self.samples]), (sz * n)(*[int(y.shape[0]) for y in self.samples]),
            (vp * n)(*[_ptr(x) for x in self.out_iq]), (vp * n)(*[_ptr(x) for x in self.out_sym]), outc,
            ctypes.byref(h)), "ChainBatchPlan")
        self._h = h
        self._prod, self._kout = (sz * n)(), (sz * n)()
        self._fn = load_library().modem_chain_batch_run

    def run(self, stream=None):
        """Returns (samples produced, kept instants produced) per channel. A launch error part-way
        through a run (ModemError, HIP) leaves some groups' handles advanced: the plan is then
        failed in the library and every later run raises too."""
        _check(self._fn(self._h, self._prod, self._kout, _stream_handle(stream, self.txs[0].device)),
               "ChainBatchPlan.run")
        for tx, rx, k, n in zip(self.txs, self.rxs, self._nb, self._prod):
            tx._ncarry = (tx._ncarry + k) % tx.bps
            tx.carrier.sample += n
            rx._consumed += n
            rx.carrier.sample += n
        return list(self._prod), list(self._kout)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.modem_chain_batch_destroy(self._h)
            self._h = None


# ------------------------------------------------------------------ channel model ----
class Channel:
    """Channel model (GLUE: the reference has none) between `DigitalModulator.process` and
    `DemodulatorRx.process`: y[n] = gain * x[n] * e^{j theta[n]} + sqrt(n0) * w[n] on (n, 2) I/Q.

    theta[n] = 2 pi ((phase0 + step n) mod 2^64) / 2^64 with the uint64 pair `nco` = (step, phase0)
    derived from `cfo` (radians per sample) and `phase` (radians); w[n] is a unit-variance complex
    Gaussian that depends only on `seed` and the absolute sample index n (`s0` plus the position in
    the stream), so any cut of a stream into calls gives the same bytes. n0 is the complex noise
    variance: pass scale = 1/n0 to the demapper and the detectors. `process(x)` takes a CUDA tensor
    (asynchronous on the current stream) or a numpy array and returns the result on the same side;
    `out=x` works in place when the dtypes are equal."""

    def __init__(self, gain: float = 1.0, phase: float = 0.0, cfo: float = 0.0, n0: float = 0.0, seed: int = 0,
                 s0: int = 0, in_dtype: int = DTYPE_F32, out_dtype: int = DTYPE_F32, device: int = 0):
        if not 0 <= int(seed) < 1 << 64 or not 0 <= int(s0) < 1 << 64:
            raise ModemPanic(ERR_INVALID_ARG, "Channel: seed and s0 are uint64")
        self.in_dtype, self.out_dtype, self.device = in_dtype, out_dtype, device
        h = ctypes.c_void_p()
        _check(load_library().modem_chan_create(float(gain), float(phase), float(cfo), float(n0), int(seed), int(s0),
                                                in_dtype, out_dtype, device, ctypes.byref(h)), "Channel")
        self._h = h

    def process(self, x, out=None, stream=None):
        n = _check_rx_input(x, self.in_dtype, "Channel.process")
        np_dtype = _LLR_DTYPE[self.out_dtype]
        y = out if out is not None else _empty_like_input(x, (n, 2), np_dtype)
        cap = _check_out(y, np_dtype, "Channel.process: out") // 2
        _check(load_library().modem_chan_process(self._h, _ptr(x), n, _ptr(y), cap,
                                                 _stream_handle(stream, self.device)), "Channel.process")
        return y

    def set_n0(self, n0: float) -> None:
        _check(load_library().modem_chan_set_n0(self._h, float(n0)), "Channel.set_n0")

    @property
    def nco(self) -> Tuple[int, int]:
        step, phase0 = ctypes.c_uint64(), ctypes.c_uint64()
        _check(load_library().modem_chan_nco(self._h, ctypes.byref(step), ctypes.byref(phase0)), "Channel.nco")
        return int(step.value), int(phase0.value)

    @property
    def sample(self) -> int:
        return int(load_library().modem_chan_sample(self._h))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.modem_chan_destroy(self._h)
            self._h = None


# ------------------------------------------------------------ carrier synchronizer ----
def _sync_params(lut, what: str = "synchronizer"):
    """(M, norm, ref_phase) of a constellation table: see _Phasor.synchronizer."""
    z = np.asarray(lut, dtype=np.float64).reshape(-1, 2)
    z = z[:, 0] + 1j * z[:, 1]
    ms = float(np.mean(np.abs(z) ** 2))
    if not ms > 0.0 or not math.isfinite(ms):
        raise ModemPanic(ERR_INVALID_ARG, f"{what}: a table without energy")
    norm = 1.0 / math.sqrt(ms)
    for power in (2, 4, 8):
        p = (norm * z) ** power
        line = complex(p.sum())
        if abs(line) / float(np.abs(p).sum()) >= 0.25:
            return power, norm, math.atan2(line.imag, line.real)
    raise ModemPanic(ERR_INVALID_ARG, f"{what}: no power of 2, 4, 8 leaves a spectral line of this constellation")


class CarrierSync:
    """Feedforward carrier synchronizer (GLUE: the reference has none) at symbol rate, on the (n, 2)
    I/Q that `DemodulatorRx.process` returns and in front of the demapper: block M-th-power phase
    estimates over `block` symbols, unwrapped across blocks, applied as a piecewise-linear
    derotation (include/modem_hip.h, "Carrier synchronizer"). `power` M in (2, 4, 8); `norm` scales
    the points before the power; `ref_phase` is the argument of sum_s (norm lut_s)^M; the tracker
    starts at `phase0`. The constellation comes out up to a multiple of 1/M turn, which `phase0`
    selects; the offset per symbol must stay below pi / (M block).

    `process(riq)` returns (out, theta, quality) for the floor((carried + n) / block) blocks the
    call completes: out (blocks * block, 2) of out_dtype, theta (blocks,) the unwrapped phase at
    each block centre in 2^-64 turns (numpy uint64, or the same bits in a torch int64), quality
    (blocks,) float32 |P| / S in [0, 1]; the < block symbols left over carry into the next call.
    `flush()` returns the carried symbols rotated on the last block's line. CUDA tensors
    (asynchronous on the current stream) or numpy arrays, results on the side of the input."""

    def __init__(self, power: int, block: int = 256, norm: float = 1.0, ref_phase: float = 0.0, phase0: float = 0.0,
                 flags: int = 0, in_dtype: int = DTYPE_F32, out_dtype: int = DTYPE_F32, device: int = 0):
        if not 0 <= int(power) < 1 << 32 or not 0 <= int(block) < 1 << 32 or not 0 <= int(flags) < 1 << 32:
            raise ModemPanic(ERR_INVALID_ARG, "CarrierSync: power, block and flags are uint32")
        self.power, self.block, self.in_dtype, self.out_dtype, self.device = int(power), int(block), in_dtype, out_dtype, device
        self.norm, self.ref_phase, self.phase0, self.flags = float(norm), float(ref_phase), float(phase0), int(flags)
        h = ctypes.c_void_p()
        _check(load_library().modem_sync_create(self.power, self.block, float(norm), float(ref_phase), float(phase0),
                                                int(flags), in_dtype, out_dtype, device, ctypes.byref(h)), "CarrierSync")
        self._h = h
        self._ncarry = 0

    def nblocks(self, n: int) -> int:
        return (self._ncarry + int(n)) // self.block

    def process(self, riq, out=None, stream=None):
        n = _check_rx_input(riq, self.in_dtype, "CarrierSync.process")
        nb = self.nblocks(n)
        np_dtype = _LLR_DTYPE[self.out_dtype]
        y = out if out is not None else _empty_like_input(riq, (nb * self.block, 2), np_dtype)
        cap = _check_out(y, np_dtype, "CarrierSync.process: out") // 2
        if _is_torch(riq):
            import torch
            theta = torch.empty(nb, dtype=torch.int64, device=riq.device)
            q = torch.empty(nb, dtype=torch.float32, device=riq.device)
        else:
            theta, q = np.empty(nb, np.uint64), np.empty(nb, np.float32)
        prod, blocks = ctypes.c_size_t(), ctypes.c_size_t()
        _check(load_library().modem_sync_process(self._h, _ptr(riq) if n else None, n, _ptr(y), cap, _ptr(theta), _ptr(q),
                                                 nb, ctypes.byref(prod), ctypes.byref(blocks),
                                                 _stream_handle(stream, self.device)), "CarrierSync.process")
        self._ncarry = (self._ncarry + n) % self.block
        p = prod.value
        return (y if int(y.shape[0]) == p else y[:p]), theta, q

    def flush(self, like=None, stream=None):
        n = self._ncarry
        ref = like if like is not None else np.zeros(1, np.float32)
        y = _empty_like_input(ref, (n, 2), _LLR_DTYPE[self.out_dtype])
        prod = ctypes.c_size_t()
        _check(load_library().modem_sync_flush(self._h, _ptr(y), n, ctypes.byref(prod),
                                               _stream_handle(stream, self.device)), "CarrierSync.flush")
        self._ncarry = 0
        return y

    @property
    def symbol(self) -> int:
        return int(load_library().modem_sync_symbol(self._h))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.modem_sync_destroy(self._h)
            self._h = None


# ------------------------------------------------------ symbol timing synchronizer ----
class TimingSync:
    """Feedforward symbol timing synchronizer (GLUE: the reference has none) at sample rate, on the
    (n, 2) I/Q that `DemodulatorRx.process` returns with decim == 1 and in front of the carrier
    synchronizer: block square-law delay estimates over `block` symbols of `sps` (4 or 8) samples,
    unwrapped across blocks, applied as a piecewise-linear delay through a cubic interpolator
    (include/modem_hip.h, "Symbol timing synchronizer"). The tracked delay stays within +-`span`
    symbols and starts at `tau0` symbols; `flat` keeps one delay per block. Output symbol k is the
    centre of the eye of grid symbol k - span.

    `process(x)` returns (out, tau, quality) for the floor((carried + n) / (block sps)) blocks the
    call completes: out (blocks * block, 2) of out_dtype, tau (blocks,) int64 the unwrapped delay of
    each block in 2^-32 symbols, quality (blocks,) float32 |X| / S in [0, 1]; the samples of the
    incomplete block carry into the next call. `flush()` returns the symbols of the incomplete
    block. CUDA tensors (asynchronous on the current stream) or numpy arrays, results on the side
    of the input."""

    def __init__(self, sps: int, block: int = 256, span: int = 2, tau0: float = 0.0, flat: bool = False,
                 in_dtype: int = DTYPE_F32, out_dtype: int = DTYPE_F32, device: int = 0):
        if not 0 <= int(sps) < 1 << 32 or not 0 <= int(block) < 1 << 32 or not 0 <= int(span) < 1 << 32:
            raise ModemPanic(ERR_INVALID_ARG, "TimingSync: sps, block and span are uint32")
        self.sps, self.block, self.span, self.tau0, self.flat = int(sps), int(block), int(span), float(tau0), bool(flat)
        self.in_dtype, self.out_dtype, self.device = in_dtype, out_dtype, device
        h = ctypes.c_void_p()
        _check(load_library().modem_timing_create(self.sps, self.block, self.span, self.tau0, 1 if flat else 0,
                                                  in_dtype, out_dtype, device, ctypes.byref(h)), "TimingSync")
        self._h = h
        self._ncarry = 0

    def nblocks(self, n: int) -> int:
        return (self._ncarry + int(n)) // (self.block * self.sps)

    def process(self, x, out=None, stream=None):
        n = _check_rx_input(x, self.in_dtype, "TimingSync.process")
        nb = self.nblocks(n)
        np_dtype = _LLR_DTYPE[self.out_dtype]
        y = out if out is not None else _empty_like_input(x, (nb * self.block, 2), np_dtype)
        cap = _check_out(y, np_dtype, "TimingSync.process: out") // 2
        if _is_torch(x):
            import torch
            tau = torch.empty(nb, dtype=torch.int64, device=x.device)
            q = torch.empty(nb, dtype=torch.float32, device=x.device)
        else:
            tau, q = np.empty(nb, np.int64), np.empty(nb, np.float32)
        prod, blocks = ctypes.c_size_t(), ctypes.c_size_t()
        _check(load_library().modem_timing_process(self._h, _ptr(x) if n else None, n, _ptr(y), cap, _ptr(tau), _ptr(q),
                                                   nb, ctypes.byref(prod), ctypes.byref(blocks),
                                                   _stream_handle(stream, self.device)), "TimingSync.process")
        self._ncarry = (self._ncarry + n) % (self.block * self.sps)
        p = prod.value
        return (y if int(y.shape[0]) == p else y[:p]), tau, q

    def flush(self, like=None, stream=None):
        n = self._ncarry // self.sps
        ref = like if like is not None else np.zeros(1, np.float32)
        y = _empty_like_input(ref, (n, 2), _LLR_DTYPE[self.out_dtype])
        prod = ctypes.c_size_t()
        _check(load_library().modem_timing_flush(self._h, _ptr(y), n, ctypes.byref(prod),
                                                 _stream_handle(stream, self.device)), "TimingSync.flush")
        self._ncarry = 0
        return y

    @property
    def sample(self) -> int:
        return int(load_library().modem_timing_sample(self._h))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.modem_timing_destroy(self._h)
            self._h = None


# --------------------------------------------------------------- frame synchronizer ----
class FrameSync:
    """Data-aided frame synchronizer (GLUE: the reference has none) at symbol rate, on the (n, 2)
    symbols that `CarrierSync.process` returns: the unique word `uw` ((L, 2) float32, 8 <= L <= 256)
    is correlated against the stream, and the peaks of the normalised correlation |c| / sqrt(e Eu)
    that reach `threshold` and dominate `guard` positions on either side (default L) are the hits
    (include/modem_hip.h, "Frame synchronizer").

    `process(x, cap=None)` returns (pos, phi, metric, count) for the positions the call decides:
    `count` (1,) the number of hits, never capped; the first min(count, cap) entries of pos (stream
    index of the unique word's first symbol; numpy uint64, or the same bits in a torch int64), phi
    (the angle of the peak as a 32-bit fraction of a turn; numpy uint32 / torch int32 bits) and
    metric (float32) are written, the rest is left as allocated. `cap` defaults to the most hits
    the call can decide. `flush()` decides what is left and starts a fresh window. `gather(x, base,
    pos, phi, count, ...)` cuts `length` symbols from `skip` after each hit out of x (whose first
    symbol is stream index `base`) and takes the nearest multiple of 1 / `power` turn to phi off:
    (frames (cap, length, 2), ok (cap,) uint8). CUDA tensors (asynchronous on the current stream,
    nothing is read back) or numpy arrays, results on the side of the input."""

    def __init__(self, uw, guard: Optional[int] = None, threshold: float = 0.6, in_dtype: int = DTYPE_F32,
                 device: int = 0):
        u = np.ascontiguousarray(np.asarray(uw, dtype=np.float32))
        if u.ndim != 2 or u.shape[1] != 2:
            raise ModemPanic(ERR_INVALID_ARG, "FrameSync: uw must be (L, 2)")
        self.uw, self.length = u, int(u.shape[0])
        self.guard = self.length if guard is None else int(guard)
        if not 0 <= self.guard < 1 << 32:
            raise ModemPanic(ERR_INVALID_ARG, "FrameSync: guard is uint32")
        self.threshold, self.in_dtype, self.device, self.power = float(threshold), in_dtype, device, 1
        h = ctypes.c_void_p()
        _check(load_library().modem_frame_create(_fptr(u), self.length, self.guard, self.threshold, in_dtype, device,
                                                 ctypes.byref(h)), "FrameSync")
        self._h = h
        self._ncarry = 0

    def _outputs(self, like, cap: int):
        if _is_torch(like):
            import torch
            dev = like.device
            return (torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                    torch.empty(cap, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int64, device=dev))
        return np.empty(cap, np.uint64), np.empty(cap, np.uint32), np.empty(cap, np.float32), np.empty(1, np.uint64)

    def process(self, x, cap: Optional[int] = None, stream=None):
        n = _check_rx_input(x, self.in_dtype, "FrameSync.process")
        if cap is None:
            cap = (self._ncarry + n) // (self.guard + 1) + 1
        pos, phi, metric, count = self._outputs(x, int(cap))
        _check(load_library().modem_frame_process(self._h, _ptr(x) if n else None, n, _ptr(pos), _ptr(phi), _ptr(metric),
                                                  int(cap), _ptr(count), _stream_handle(stream, self.device)),
               "FrameSync.process")
        self._ncarry = min(self._ncarry + n, 2 * self.guard + self.length - 1)
        return pos, phi, metric, count

    def flush(self, like=None, cap: Optional[int] = None, stream=None):
        if cap is None:
            cap = self._ncarry // (self.guard + 1) + 1
        pos, phi, metric, count = self._outputs(like if like is not None else np.zeros(1, np.float32), int(cap))
        _check(load_library().modem_frame_flush(self._h, _ptr(pos), _ptr(phi), _ptr(metric), int(cap), _ptr(count),
                                                _stream_handle(stream, self.device)), "FrameSync.flush")
        self._ncarry = 0
        return pos, phi, metric, count

    def gather(self, x, base: int, pos, phi, count, skip: Optional[int] = None, length: int = 1,
               power: Optional[int] = None, out_dtype: int = DTYPE_F32, stream=None):
        n = _check_rx_input(x, self.in_dtype, "FrameSync.gather")
        cap = int(pos.shape[0])
        if phi is not None and int(phi.shape[0]) != cap:
            raise ModemPanic(ERR_INVALID_ARG, "FrameSync.gather: pos and phi differ in size")
        if not 0 <= int(base) < 1 << 64:
            raise ModemPanic(ERR_INVALID_ARG, "FrameSync.gather: base is uint64")
        skip = self.length if skip is None else int(skip)
        power = self.power if power is None else int(power)
        if not 0 <= skip < 1 << 32 or not 0 <= int(length) < 1 << 32 or not 0 <= power < 1 << 32:
            raise ModemPanic(ERR_INVALID_ARG, "FrameSync.gather: skip, length and power are uint32")
        np_dtype = _LLR_DTYPE[out_dtype]
        frames = _empty_like_input(x, (cap, int(length), 2), np_dtype)
        ok = _empty_like_input(x, (cap,), np.uint8)
        _check(load_library().modem_frame_gather(_ptr(x) if n else None, n, int(base), _ptr(pos), _ptr(phi), _ptr(count),
                                                 cap, skip, int(length), power, self.in_dtype, out_dtype,
                                                 _ptr(frames), _ptr(ok), self.device,
                                                 _stream_handle(stream, self.device)), "FrameSync.gather")
        return frames, ok

    @property
    def symbol(self) -> int:
        return int(load_library().modem_frame_symbol(self._h))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.modem_frame_destroy(self._h)
            self._h = None


# ---------------------------------------------------------------- convolutional code ----
class ConvCode:
    """A rate-1/n convolutional code (GLUE: the reference has none; include/modem_hip.h,
    "Convolutional code"): constraint length 3 <= K <= 9, n = 2 or 3 generator polynomials whose top
    bit taps the current input bit (the usual octal notation; the default is the customary K = 7
    pair), and with `tail` K-1 zero bits that end every frame in state 0.

    `encode(bits)` takes (nframes, nbits) uint8 on the device, one bit per byte (only bit 0 counts),
    and returns the (nframes, n T) coded bits, T = nbits + K - 1 with the tail, as
    `DigitalModulator.process` takes them once flattened. `coded_bits(nbits)` is n T.
    `decoder(in_dtype)` is the `ViterbiDecoder` of the code."""

    def __init__(self, K: int = 7, polys: Sequence[int] = (0o171, 0o133), tail: bool = True):
        self.K, self.polys, self.tail = int(K), tuple(int(g) for g in polys), bool(tail)
        self.n = len(self.polys)
        if not 3 <= self.K <= 9 or self.n not in (2, 3) or any(not 0 < g < 1 << self.K for g in self.polys):
            raise ModemPanic(ERR_INVALID_ARG, f"ConvCode: K = {K}, polys = {polys}")
        self.flags = CONV_TAIL if self.tail else 0

    def _polys(self):
        return (ctypes.c_uint32 * self.n)(*self.polys)

    def steps(self, nbits: int) -> int:
        return int(nbits) + (self.K - 1 if self.tail else 0)

    def coded_bits(self, nbits: int) -> int:
        return self.n * self.steps(nbits)

    def encode(self, bits, out=None, stream=None):
        if not _is_torch(bits) or not bits.is_cuda or bits.dim() != 2 or _dtype_name(bits) != "uint8":
            raise ValueError("ConvCode.encode: bits must be a 2-D uint8 CUDA tensor")
        import torch
        nframes, nbits = int(bits.shape[0]), int(bits.shape[1])
        ncoded = self.coded_bits(nbits)
        if out is None:
            out = torch.empty((nframes, ncoded), dtype=torch.uint8, device=bits.device)
        elif _dtype_name(out) != "uint8" or out.dim() != 2 or int(out.shape[0]) != nframes or int(out.shape[1]) < ncoded:
            raise ValueError(f"ConvCode.encode: out must be uint8 ({nframes}, >= {ncoded})")
        device = _device_of(bits, 0)
        _check(load_library().modem_conv_encode(self.K, self._polys(), self.n, self.flags, _ptr(bits) if nframes else None,
                                                nframes, nbits, nbits, _ptr(out) if nframes else None, int(out.shape[1]),
                                                device, _stream_handle(stream, device)), "ConvCode.encode")
        return out

    def decoder(self, in_dtype: int = DTYPE_I8, device: int = 0) -> "ViterbiDecoder":
        return ViterbiDecoder(self, in_dtype=in_dtype, device=device)

    def rate_match(self, pattern: Sequence[int] = (1,), cols: int = 1, device: int = 0) -> "RateMatch":
        """The `RateMatch` of a puncturing pattern over the code's bits (index t*n + j) and an interleaver."""
        return RateMatch(pattern, cols=cols, device=device)


class ViterbiDecoder:
    """Batched soft-decision Viterbi decoder of a `ConvCode` on the demapper's LLRs (positive =
    "bit 0"), int8 (the default), float16 or float32; float input is quantised to integers in
    +-127 as rint(clamp(llr * qscale)). Metrics are integers: the output is specified bit for bit.

    `process(llr, nbits, stride=None, ok=None, qscale=1.0, want_metric=True)` -> (bits, metric):
    `llr` is a CUDA tensor: 2-D (nframes, >= n T), or of any shape with `stride` (elements between
    frames), or frames of n T values back to back, so that the demapper's (nsym, bps) output over
    `frames.view(-1, 2)` passes straight in; `ok` the (nframes,)
    uint8 flags of `FrameSync.gather` or None: a frame with ok == 0 is not decoded, its bits and
    metric are 0. bits is (nframes, nbits) uint8, metric (nframes,) int32 (the final correlation) or
    None. Asynchronous on the current stream; nothing is read back. A frame may have at most 4096
    steps (2048 for K = 8, 1024 for K = 9)."""

    def __init__(self, code: ConvCode, in_dtype: int = DTYPE_I8, device: int = 0):
        self.code, self.in_dtype, self.device = code, in_dtype, device
        h = ctypes.c_void_p()
        _check(load_library().modem_viterbi_create(code.K, code._polys(), code.n, code.flags, in_dtype, device,
                                                   ctypes.byref(h)), "ViterbiDecoder")
        self._h = h

    def process(self, llr, nbits: int, stride: Optional[int] = None, ok=None, qscale: float = 1.0,
                want_metric: bool = True, stream=None):
        if not _is_torch(llr) or not llr.is_cuda:
            raise ValueError("ViterbiDecoder.process: llr must be a CUDA tensor")
        if _dtype_name(llr) != np.dtype(_LLR_DTYPE[self.in_dtype]).name:
            raise ValueError(f"ViterbiDecoder.process: llr must be {np.dtype(_LLR_DTYPE[self.in_dtype]).name} "
                             f"(the handle's in_dtype), got {_dtype_name(llr)}")
        import torch
        nbits = int(nbits)
        ncoded = self.code.coded_bits(nbits)
        total = int(llr.numel())
        if stride is not None:
            stride = int(stride)
            if stride <= 0:
                raise ValueError("ViterbiDecoder.process: stride must be positive")
            nframes = 0 if total < ncoded else (total - ncoded) // stride + 1
        elif llr.dim() == 2 and int(llr.shape[1]) >= ncoded:
            nframes, stride = int(llr.shape[0]), int(llr.shape[1])
        elif total % ncoded == 0:                          # frames back to back, e.g. the demapper's (nsym, bps)
            nframes, stride = total // ncoded, ncoded
        else:
            raise ValueError(f"ViterbiDecoder.process: {total} values are not whole frames of {ncoded}; give a stride")
        if ok is not None:
            if not _is_torch(ok) or _dtype_name(ok) != "uint8" or int(ok.numel()) != nframes:
                raise ValueError(f"ViterbiDecoder.process: ok must be {nframes} uint8 flags on the device")
        bits = torch.empty((nframes, nbits), dtype=torch.uint8, device=llr.device)
        metric = torch.empty((nframes,), dtype=torch.int32, device=llr.device) if want_metric else None
        _check(load_library().modem_viterbi_process(self._h, _ptr(llr) if nframes else None, stride, nframes, nbits,
                                                    float(qscale), _ptr(ok), _ptr(bits) if nframes else None, nbits,
                                                    _ptr(metric), _stream_handle(stream, self.device)),
               "ViterbiDecoder.process")
        return bits, metric

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.modem_viterbi_destroy(self._h)
            self._h = None


# ------------------------------------------------------ rate matching and frame check ----
PUNCTURE_2_3 = (1, 1, 1, 0)                 # K = 7 (0171, 0133), coded bit t*n + j: rate 2/3
PUNCTURE_3_4 = (1, 1, 1, 0, 0, 1)           # rate 3/4


def _rows(x, names, what: str):
    """(nframes, ncols, row stride in elements) of a 2-D CUDA tensor whose rows are contiguous: the
    rows may be a view into a wider buffer (x = buf[:, :ncols]), and the stride is the tensor's."""
    if not _is_torch(x) or not x.is_cuda or x.dim() != 2 or _dtype_name(x) not in names:
        raise ValueError(f"{what} must be a 2-D CUDA tensor of {' / '.join(names)}")
    nframes, ncols = int(x.shape[0]), int(x.shape[1])
    if ncols and int(x.stride(1)) != 1:
        raise ValueError(f"{what}: the elements of a row must be contiguous")
    stride = int(x.stride(0)) if nframes > 1 else ncols
    if stride < ncols:
        raise ValueError(f"{what}: rows overlap (stride {stride} < {ncols})")
    return nframes, ncols, stride


class RateMatch:
    """Puncturing and a pruned block interleaver between `ConvCode.encode` and the modulator, and
    their inverse between the demapper and the `ViterbiDecoder` (GLUE: the reference has none;
    include/modem_hip.h, "Rate matching and frame check").

    `pattern`: 1 .. 64 values 0 / 1, at least one 1; mother index m of a frame is kept iff
    pattern[m mod P] == 1 (`PUNCTURE_2_3`, `PUNCTURE_3_4` for the K = 7 pair). `cols`: 1 .. 256
    columns of the interleaver over the kept values of a frame; 1 is none. `kept(nm)` is E, the
    values of a frame of nm mother indices that are transmitted.
    `tx(coded)`: (nframes, nm) uint8 -> (nframes, E) uint8, as `DigitalModulator.process` takes them
    once flattened. `rx(llr, nm)`: (nframes, E) int8 / float16 / float32 -> (nframes, nm) of the same
    dtype, every value moved as it is, a punctured position +0 (the decoder's erasure). Rows may be
    views into wider buffers (the row stride is the tensor's); `out` likewise, and nothing is
    written outside its rows. Asynchronous on `stream` (default: the current one)."""

    PUNCTURE_2_3, PUNCTURE_3_4 = PUNCTURE_2_3, PUNCTURE_3_4

    def __init__(self, pattern: Sequence[int] = (1,), cols: int = 1, device: int = 0):
        self.pattern, self.cols, self.device = tuple(int(v) for v in pattern), int(cols), int(device)
        if not 1 <= len(self.pattern) <= 64 or any(v not in (0, 1) for v in self.pattern) or not any(self.pattern):
            raise ModemPanic(ERR_INVALID_ARG, f"RateMatch: pattern = {pattern}")
        if not 1 <= self.cols <= 256:
            raise ModemPanic(ERR_INVALID_ARG, f"RateMatch: cols = {cols}")
        self._pat = (ctypes.c_uint8 * len(self.pattern))(*self.pattern)

    def kept(self, nm: int) -> int:
        e = ctypes.c_size_t(0)
        _check(load_library().modem_rm_kept(self._pat, len(self.pattern), int(nm), ctypes.byref(e)), "RateMatch.kept")
        return int(e.value)

    def _out(self, out, ref, nframes, ncols, dtype, what):
        if out is None:
            import torch
            return torch.empty((nframes, ncols), dtype=dtype, device=ref.device), ncols
        n, c, stride = _rows(out, (_dtype_name(ref),), f"{what}: out")
        if n != nframes or c < ncols or out.device != ref.device:
            raise ValueError(f"{what}: out must be ({nframes}, >= {ncols}) on the input's device")
        return out, stride

    def tx(self, coded, out=None, stream=None):
        nframes, nm, stride = _rows(coded, ("uint8",), "RateMatch.tx: coded")
        e = self.kept(nm)
        out, ostride = self._out(out, coded, nframes, e, coded.dtype, "RateMatch.tx")
        device = _device_of(coded, self.device)
        _check(load_library().modem_rm_tx(self._pat, len(self.pattern), self.cols, int(coded.data_ptr()) if nframes else None,
                                          nframes, nm, stride, int(out.data_ptr()) if nframes else None, ostride, device,
                                          _stream_handle(stream, device)), "RateMatch.tx")
        return out

    def rx(self, llr, nm: int, out=None, stream=None, ok=None):
        nframes, e, stride = _rows(llr, ("int8", "float16", "float32"), "RateMatch.rx: llr")
        nm = int(nm)
        if e != self.kept(nm):
            raise ValueError(f"RateMatch.rx: rows of {e} values, but {self.kept(nm)} of {nm} are kept")
        if ok is not None and (not _is_torch(ok) or _dtype_name(ok) != "uint8" or int(ok.numel()) != nframes):
            raise ValueError(f"RateMatch.rx: ok must be {nframes} uint8 flags on the device")
        dtype = {"int8": DTYPE_I8, "float16": DTYPE_F16, "float32": DTYPE_F32}[_dtype_name(llr)]
        out, ostride = self._out(out, llr, nframes, nm, llr.dtype, "RateMatch.rx")
        device = _device_of(llr, self.device)
        _check(load_library().modem_rm_rx(self._pat, len(self.pattern), self.cols, dtype, int(llr.data_ptr()) if nframes else None,
                                          nframes, nm, stride, _ptr(ok), int(out.data_ptr()) if nframes else None, ostride,
                                          device, _stream_handle(stream, device)), "RateMatch.rx")
        return out


class CRC:
    """A CRC over the bits of a frame, one byte per bit (GLUE; include/modem_hip.h, "Rate matching and
    frame check"): width 8, 16, 24 or 32, `poly` with the top bit implicit, `init`, `xorout`, no
    reflection, the first bit of a row first. `attach(bits)`: (nframes, nbits) uint8 -> (nframes,
    nbits + width): the bits, then the CRC, most significant bit first. `check(bits, ok=None)`:
    (nframes, nbits + width) uint8 -> ok' (nframes,) uint8: 1 iff the trailing width bits are the
    CRC of the bits before them and `ok` (the flags the decoder got; None: all ones) is not 0;
    `out` may be `ok` itself. Only bit 0 of a byte counts. Asynchronous on `stream`; nothing is
    read back."""

    def __init__(self, width: int, poly: int, init: int = 0, xorout: int = 0):
        self.width, self.poly, self.init, self.xorout = int(width), int(poly), int(init), int(xorout)
        if self.width not in (8, 16, 24, 32) or any(not 0 <= v < 1 << self.width for v in (self.poly, self.init, self.xorout)):
            raise ModemPanic(ERR_INVALID_ARG, f"CRC: width = {width}, poly = {poly:#x}, init = {init:#x}, xorout = {xorout:#x}")

    @classmethod
    def ccitt16(cls) -> "CRC":
        return cls(16, 0x1021, 0xFFFF)

    @classmethod
    def mpeg32(cls) -> "CRC":
        return cls(32, 0x04C11DB7, 0xFFFFFFFF)

    def attach(self, bits, out=None, stream=None):
        nframes, nbits, stride = _rows(bits, ("uint8",), "CRC.attach: bits")
        if out is None:
            import torch
            out, ostride = torch.empty((nframes, nbits + self.width), dtype=torch.uint8, device=bits.device), nbits + self.width
        else:
            n, c, ostride = _rows(out, ("uint8",), "CRC.attach: out")
            if n != nframes or c < nbits + self.width or out.device != bits.device:
                raise ValueError(f"CRC.attach: out must be uint8 ({nframes}, >= {nbits + self.width}) on the input's device")
        device = _device_of(bits, 0)
        _check(load_library().modem_crc_attach(self.width, self.poly, self.init, self.xorout,
                                               int(bits.data_ptr()) if nframes else None, nframes, nbits, stride,
                                               int(out.data_ptr()) if nframes else None, ostride, device,
                                               _stream_handle(stream, device)), "CRC.attach")
        return out

    def check(self, bits, ok=None, out=None, stream=None):
        nframes, ncols, stride = _rows(bits, ("uint8",), "CRC.check: bits")
        if ncols <= self.width:
            raise ModemPanic(ERR_INVALID_ARG, f"CRC.check: rows of {ncols} bytes hold no message in front of {self.width} CRC bits")
        for name, t in (("ok", ok), ("out", out)):
            if t is not None and (not _is_torch(t) or not t.is_cuda or _dtype_name(t) != "uint8" or int(t.numel()) != nframes):
                raise ValueError(f"CRC.check: {name} must be {nframes} uint8 flags on the device")
        if out is None:
            import torch
            out = torch.empty((nframes,), dtype=torch.uint8, device=bits.device)
        device = _device_of(bits, 0)
        _check(load_library().modem_crc_check(self.width, self.poly, self.init, self.xorout,
                                              int(bits.data_ptr()) if nframes else None, nframes, ncols - self.width, stride,
                                              _ptr(ok), _ptr(out) if nframes else None, device,
                                              _stream_handle(stream, device)), "CRC.check")
        return out


def count_errors(a, b, counts=None, stream=None, device: int = 0):
    """counts[0] += #{i: a[i] != b[i]}, counts[1] += sum_i popcount(a[i] ^ b[i]) over two uint8
    buffers of one size (bits, one byte each, or symbols), both CUDA tensors (asynchronous on the
    current stream; no host copy) or both numpy arrays. `counts`: a 2-element int64 tensor / array
    on the same side to accumulate into, or None for a new one, zeroed on the stream of the call
    (`stream`, else the current one). Returns it."""
    if _is_torch(a) != _is_torch(b) or (counts is not None and _is_torch(counts) != _is_torch(a)):
        raise ModemPanic(ERR_INVALID_ARG, "count_errors: a, b and counts must be on one side")
    n = _check_out(a, np.uint8, "count_errors: a")
    if _check_out(b, np.uint8, "count_errors: b") != n:
        raise ModemPanic(ERR_INVALID_ARG, "count_errors: a and b differ in size")
    if counts is None:
        if _is_torch(a):
            import torch
            if stream is None:
                counts = torch.zeros(2, dtype=torch.int64, device=a.device)
            else:
                # the zero-fill must be ordered before the kernel: queue it on the kernel's stream,
                # not on torch's current one
                s = stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(int(stream), device=a.device)
                with torch.cuda.stream(s):
                    counts = torch.zeros(2, dtype=torch.int64, device=a.device)
        else:
            counts = np.zeros(2, dtype=np.int64)
    elif _check_out(counts, np.int64, "count_errors: counts") != 2:
        raise ModemPanic(ERR_INVALID_ARG, "count_errors: counts must have 2 elements")
    device = _device_of(a, device)
    _check(load_library().modem_count_errors(_ptr(a) if n else None, _ptr(b) if n else None, n, _ptr(counts), device,
                                             _stream_handle(stream, device)), "count_errors")
    return counts


def prng_bits(seed: int, nbits: int, device: int = 0, stream=None):
    """Synthetic bit stream (GLUE): splitmix64, one byte per bit, on the device."""
    import torch
    out = torch.empty(int(nbits), dtype=torch.uint8, device=f"cuda:{device}")
    _check(load_library().modem_prng_bits(int(seed), out.data_ptr() if nbits else None, int(nbits), device,
                                          _stream_handle(stream, device)), "prng_bits")
    return out
