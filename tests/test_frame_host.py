"""Frame synchronizer, host side (no device needed): the C ABI entry points exist and refuse bad
arguments before they look for a device; the rotation index at every branch boundary; the two
consequences of the peak rule on the restatement; every random-input case of tests/test_gpu_frame.py
free of borderline positions; and the restatements alone on the oracle's loopback, which must meet
the conditions tests/test_gpu_frame_loopback.py puts on the device."""
import ctypes

import numpy as np
import pytest

import chan_ref
import frame_ref
import sync_ref

BAD_DEVICE = 1 << 20
SYMBOLS = ("modem_frame_create", "modem_frame_process", "modem_frame_flush", "modem_frame_symbol", "modem_frame_destroy",
           "modem_frame_gather")


def _uw(L=16):
    rng = np.random.RandomState(1)
    return np.ascontiguousarray(rng.choice([-1.0, 1.0], (L, 2)).astype(np.float32))


def _create(m, uw="default", length=None, guard=8, threshold=0.6, in_dtype=0, device=0, out="handle"):
    u = _uw() if isinstance(uw, str) else uw
    h = ctypes.c_void_p(0xDEAD)
    ptr = None if u is None else u.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    n = length if length is not None else (0 if u is None else len(u))
    st = m.load_library().modem_frame_create(ptr, n, guard, threshold, in_dtype, device,
                                             None if out is None else ctypes.byref(h))
    return st, h


def test_library_exports_the_frame_synchronizer(m):
    lib = ctypes.CDLL(m.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert m.load_library().modem_abi_version() == 6      # additive: the version stays
    assert "FrameSync" in m.__all__ and hasattr(m, "FrameSync")
    assert hasattr(m.QPSK(0.0, 1.0), "framer")


@pytest.mark.parametrize("device", [0, BAD_DEVICE])
def test_create_refusals_come_before_the_device(m, device):
    inf, nan = float("inf"), float("nan")
    big = np.ones((300, 2), np.float32)
    bad_uw = []
    for v in (nan, inf, -inf):
        u = _uw()
        u[3, 1] = v
        bad_uw.append(u)
    bad = [dict(uw=None, length=16), dict(length=0), dict(length=7), dict(uw=big, length=257), dict(uw=big, length=300),
           dict(guard=0), dict(guard=257), dict(guard=1 << 31),
           dict(threshold=0.0), dict(threshold=-0.5), dict(threshold=1.0000001), dict(threshold=nan), dict(threshold=inf),
           dict(uw=np.zeros((16, 2), np.float32)), *[dict(uw=u) for u in bad_uw],
           dict(in_dtype=m.DTYPE_I16), dict(in_dtype=m.DTYPE_I8), dict(in_dtype=-1), dict(in_dtype=4)]
    for kw in bad:
        st, h = _create(m, device=device, **kw)
        assert st == m.ERR_INVALID_ARG, kw
        assert h.value is None, kw
    st, _ = _create(m, device=device, out=None)
    assert st == m.ERR_INVALID_ARG
    for kw in (dict(guard=0), dict(threshold=0.0), dict(in_dtype=m.DTYPE_I8)):
        with pytest.raises(m.ModemPanic):
            m.FrameSync(_uw(), **{"device": device, **kw})
    with pytest.raises(m.ModemPanic):
        m.FrameSync(np.zeros((16, 2), np.float32), device=device)
    with pytest.raises(m.ModemPanic):
        m.QPSK(0.0, 1.0).framer([0, 1, 2, 4] * 4, device=device)           # a symbol outside the table
    with pytest.raises(m.ModemError):
        m.DMPSK(2, 1.0, 0.0, 1.5707964).framer([0] * 16, device=device)


def test_a_bad_ordinal_is_no_device(m):
    """The handle owns device memory, so a valid description on a device that does not exist is
    NO_DEVICE (every argument refusal above came first)."""
    for device in (BAD_DEVICE, -1):
        st, h = _create(m, device=device)
        assert st == m.ERR_NO_DEVICE and h.value is None
        st, h = _create(m, uw=_uw(256), guard=256, threshold=1.0, in_dtype=m.DTYPE_F16, device=device)
        assert st == m.ERR_NO_DEVICE and h.value is None


def test_null_handles_and_gather_refusals(m):
    L = m.load_library()
    x = np.zeros((8, 2), np.float32)
    pos, phi, met, cnt = np.zeros(4, np.uint64), np.zeros(4, np.uint32), np.zeros(4, np.float32), np.zeros(1, np.uint64)
    a = lambda v: v.ctypes.data
    assert L.modem_frame_process(None, a(x), 8, a(pos), a(phi), a(met), 4, a(cnt), None) == m.ERR_INVALID_ARG
    assert L.modem_frame_flush(None, a(pos), a(phi), a(met), 4, a(cnt), None) == m.ERR_INVALID_ARG
    assert L.modem_frame_symbol(None) == 0 and L.modem_frame_destroy(None) == m.MODEM_OK
    out, ok = np.zeros((4, 2, 2), np.float32), np.zeros(4, np.uint8)

    def gather(device, power=4, in_dtype=0, out_dtype=0, length=2, pos_=pos, cnt_=cnt, out_=out, ok_=ok):
        return L.modem_frame_gather(a(x), 8, 0, None if pos_ is None else a(pos_), a(phi), None if cnt_ is None else a(cnt_),
                                    4, 0, length, power, in_dtype, out_dtype, None if out_ is None else a(out_),
                                    None if ok_ is None else a(ok_), device, None)
    for device in (0, BAD_DEVICE):
        for kw in (dict(power=0), dict(power=3), dict(power=16), dict(in_dtype=m.DTYPE_I16), dict(out_dtype=m.DTYPE_I8),
                   dict(length=0), dict(pos_=None), dict(cnt_=None), dict(out_=None), dict(ok_=None)):
            assert gather(device, **kw) == m.ERR_INVALID_ARG, kw
    assert gather(BAD_DEVICE) == m.ERR_NO_DEVICE


def test_framer_takes_its_power_from_the_table(m):
    """power is what the gather rotates by: the M of synchronizer(); no device is needed to derive it."""
    for ph, power in ((m.BPSK(0.7853982, 1.0), 2), (m.QPSK(0.0, 1.0), 4), (m.QAM(4, 0.0, 1.0), 4), (m.MPSK(3, 0.0, 1.0), 8)):
        assert m._sync_params(ph.lut())[0] == power


@pytest.mark.parametrize("power", [2, 4, 8])
def test_rotation_index_at_every_branch_boundary(power):
    """rot is the nearest multiple of 1/M turn: the boundary phi = (2 r + 1) / (2 M) turn belongs to
    r + 1, the value before it to r; wrapping at the top."""
    step = (1 << 32) // power
    assert frame_ref.rot_of(0, 1) == 0 and frame_ref.rot_of(0xFFFFFFFF, 1) == 0
    for r in range(power):
        edge = r * step + step // 2
        assert frame_ref.rot_of(edge - 1, power) == r
        assert frame_ref.rot_of(edge, power) == (r + 1) % power
        assert frame_ref.rot_of(edge + 1, power) == (r + 1) % power
        assert frame_ref.rot_of(r * step, power) == r
        assert frame_ref.rot_of((r * step - 1) & 0xFFFFFFFF, power) == r
        lm = power.bit_length() - 1                                    # the header's expression in uint32 arithmetic
        for phi in (edge - 1, edge, edge + 1, r * step):
            with np.errstate(over="ignore"):
                assert int((np.uint32(phi) + np.uint32(1 << (31 - lm))) >> np.uint32(32 - lm)) == frame_ref.rot_of(phi, power)


def test_hits_are_more_than_guard_apart_and_the_earliest_maximum_wins():
    rng = np.random.RandomState(5)
    u = rng.choice([-1.0, 1.0], (8, 2)).astype(np.float32)
    for W in (1, 3, 8):
        x = rng.choice([-1.0, 0.0, 1.0], (600, 2)).astype(np.float32)
        for s in (0, 40, 40 + W, 100, 100 + W + 1, 300, 308, 316, 592):
            x[s:s + 8] = u
        r = frame_ref.detect(x, u, W, 0.5)
        assert len(r["pos"]) >= 4
        assert all(b - a > W for a, b in zip(r["pos"], r["pos"][1:]))
    x = np.zeros((100, 2), np.float32)
    x[10:50] = np.tile(u, (5, 1))                                      # five unique words back to back: equal maxima
    r = frame_ref.detect(x, u, 8, 0.9)
    assert r["m"][10] == r["m"][18] == r["m"][42] == r["m"].max()
    assert r["pos"] == [10]                                            # each later one has an equal maximum 8 before it


@pytest.mark.parametrize("name", list(frame_ref.NOISY))
def test_noisy_cases_have_no_borderline_position(m, name):
    """Zero is a condition: the device may then be held to the restatement's hits exactly."""
    x, u = frame_ref.noisy_case(m, name)
    r = frame_ref.detect(x, u, len(u), frame_ref.NOISY_THR)
    others = np.delete(r["metric_all"], r["pos"])
    print(f"{name}: hits {r['pos']}, metric {np.round(r['metric'], 4)}, max elsewhere {others.max():.3f}, "
          f"borderline {r['borderline']}")
    assert r["borderline"] == []
    assert r["pos"] == list(frame_ref.NOISY_STARTS)


# ------------------------------------------------- the loopback conditions, on the CPU ----
def _oracle_loopback(m, o, kind, ebn0_db):
    """The oracle's TX, chan_ref.channel with the product's NCO integers, the oracle's RX, the
    restatement of the carrier synchronizer with phase0 = 0 (flush included)."""
    C = frame_ref.LOOP
    sps, L = C["sps"], C["L"]
    taps = m.rrc_taps(L, sps, 0.35)
    w = o.sample_freq(1, 4)
    phasor = (lambda: o.new_phasor(o.QPSK, 0.0, 1.0)) if kind == "qpsk" else (lambda: o.new_phasor(o.QAM, 4, 0.0, 1.0))
    lut = o.phasor_lut(phasor())
    bps = int(lut.shape[0]).bit_length() - 1
    bits, starts, uw = frame_ref.loop_stream(o.prng_bits, bps)
    n0 = sync_ref.loop_n0(lut, ebn0_db)
    x = o.tx_chain(phasor(), bits, sps, taps, w, 0, flush_syms=(L - 1 + sps - 1) // sps)
    nco = m.Channel(cfo=C["cfo"], phase=C["phase"], device=BAD_DEVICE).nco
    y, _ = chan_ref.channel(x, nco=nco, n0=n0, seed=C["noise_seed"])
    riq, _ = o.rx_chain(y.astype(np.float32), w, 0, o.MIX_COMPLEX, taps, sps, L - 1, None)
    nsym = len(bits) // bps
    power, norm, ref = m._sync_params(lut)
    s = sync_ref.sync(riq[:nsym], power, C["block"], norm, sync_ref.turns(m, ref), 0)
    return s["out"].astype(np.float32), bits, starts, uw, lut, power


def _payload_errors(frames, lut, sent_bits, bps):
    t = frame_ref.cplx(lut)
    dec = np.argmin(np.abs(frames.reshape(-1)[:, None] - t[None, :]), 1)
    got = ((dec[:, None] >> np.arange(bps)[::-1]) & 1).astype(np.uint8).reshape(-1)
    return int((got != sent_bits.reshape(-1)).sum())


def _loopback(m, o, kind, ebn0_db):
    C = frame_ref.LOOP
    out, bits, starts, uw, lut, power = _oracle_loopback(m, o, kind, ebn0_db)
    bps = int(lut.shape[0]).bit_length() - 1
    r = frame_ref.detect(out, lut[uw], C["guard"], C["threshold"])
    others = np.delete(r["metric_all"], r["pos"])
    phi = [int(round(t * 2.0 ** 32)) & 0xFFFFFFFF for t in r["turn"]]
    sent = frame_ref.payload_bits(bits, starts, bps)
    fr, ok = frame_ref.gather(out, 0, r["pos"], phi, len(r["pos"]), C["uw"], C["payload"], power)
    fr0, _ = frame_ref.gather(out, 0, r["pos"], None, len(r["pos"]), C["uw"], C["payload"], power)
    errors = _payload_errors(fr, lut, sent, bps) if r["pos"] == starts else None
    plain = _payload_errors(fr0, lut, sent, bps) if r["pos"] == starts else None
    print(f"reference {kind} frame loopback: {len(r['pos'])} hits of {len(starts)} sent, min metric at a hit "
          f"{r['metric'].min():.3f}, max elsewhere {others.max():.3f}, borderline {r['borderline']}, rot "
          f"{sorted(set(frame_ref.rot_of(p, power) for p in phi))}, payload bit errors {errors} of {sent.size}, "
          f"without the rotation {plain}")
    return r, starts, others, errors, plain, sent.size, ok


def test_reference_meets_the_qpsk_loopback_conditions(m, o):
    """(a)-(d) of tests/test_gpu_frame_loopback.py on the oracle's chain with the restatements alone."""
    C = frame_ref.LOOP
    r, starts, others, errors, plain, nbits, ok = _loopback(m, o, "qpsk", C["qpsk_ebn0_db"])
    assert r["pos"] == starts and len(starts) == 64 and ok.all()                     # (a)
    assert r["metric"].min() >= 0.8 and others.max() <= 0.5                           # (b)
    assert r["borderline"] == []
    want, band = sync_ref.ber_band(nbits, C["qpsk_ebn0_db"])
    assert abs(errors - want) <= band                                                 # (c)
    assert plain > 0.25 * nbits                                                       # (d)


def test_reference_meets_the_qam16_loopback_conditions(m, o):
    """(e): QAM16 at 12 dB meets (a) and (b), and its bit errors are below 1 %."""
    C = frame_ref.LOOP
    r, starts, others, errors, plain, nbits, ok = _loopback(m, o, "qam16", C["qam_ebn0_db"])
    assert r["pos"] == starts and len(starts) == 64 and ok.all()
    assert r["metric"].min() >= 0.8 and others.max() <= 0.5
    assert r["borderline"] == []
    assert errors < 0.01 * nbits
