"""The device's scanned-phasor states (tx_scan / tx_scan_batch: scan_bank and scan_step<KIND> in
rust-modem_amd/csrc/modem_tx.hip and modem_scan_step.h), read back with
DigitalModulator.scan_states (modem_tx_scan_states), against the oracle's per-symbol sequence
(or_phasor_update, cross-checked by a numpy restatement in tests/test_scan_states.py) bit for bit:
every comparison of states is np.array_equal on the uint32 view. DMPSK compares column 0 (its y is
unspecified), MFSK and BFSK both columns.

The output samples cannot stand in for this: a floor that is off by one in the division-free
mod_trig moves a state by 2 pi, or by a few ulp after the next reduction, and its sine and cosine
stay within the sample tolerance (tests/test_stateful.py). tests/test_scan_states.py shows, on the
CPU, that the streams used here do expose such a step.
"""
import ctypes
import functools

import numpy as np
import pytest

import scan_ref as ref

pytestmark = pytest.mark.gpu

HZ, SR = 1000, 10000          # the carrier (it only enters the samples through out_mode; the states never)

# Symbols per call of the chunked run: the 16-symbol read-ahead and the 64-symbol LDS block of
# scan_bank, each at -1, 0 and +1; an empty call; two blocks and one symbol; then the rest.
CALLS = (1, 15, 16, 17, 63, 64, 65, 0, 129)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _mod(m, w, s0, spec):
    return m.DigitalModulator(m.Carrier(w, s0), ref.product_phasor(m, spec), ref.SPS, None, out_mode=1)


@pytest.mark.parametrize("s0", ref.S0S)
@pytest.mark.parametrize("name", list(ref.KINDS))
def test_single_channel_states_bitwise(m, o, torch_cuda, name, s0):
    """One handle fed in calls of CALLS symbols (the first leaves one bit over where a symbol has
    more than one, the second takes it up), then the rest: the states read after every call,
    concatenated, are the oracle's; one call over the whole stream gives the same states and the
    same samples bit for bit; and those samples are within the f32 sample tolerance of the oracle's
    at every carrier start (the phase argument is bitwise the oracle's once the states are)."""
    torch = torch_cuda
    spec = ref.KINDS[name]
    bps, cols = ref.bps_of(spec), ref.COLUMNS[spec[0]]
    bits, want = ref.case(name, s0)
    w = o.sample_freq(HZ, SR)
    extra = 1 if bps > 1 else 0
    nbits = [bps * k for k in CALLS]
    nbits[0] += extra
    nbits[1] -= extra
    nbits.append(len(bits) - sum(nbits))
    nsyms = list(CALLS) + [ref.NSYM - sum(CALLS)]

    tx = _mod(m, w, s0, spec)
    states, samples, pos = [], [], 0
    for nb, ns in zip(nbits, nsyms):
        samples.append(tx.process(torch.from_numpy(bits[pos:pos + nb].copy()).cuda()))
        st = tx.scan_states()
        assert st.shape == (ns, 2) and st.dtype == np.float32, (nb, ns, st.shape)
        states.append(st)
        pos += nb
    assert pos == len(bits)
    states = np.concatenate(states)
    assert ref.same_bits(states, want, cols), ref.first_difference(states, want, cols)

    one = _mod(m, w, s0, spec)
    y = one.process(torch.from_numpy(bits.copy()).cuda()).cpu().numpy()
    st1 = one.scan_states()
    assert ref.same_bits(st1, want, cols), ref.first_difference(st1, want, cols)
    assert np.array_equal(_u32(torch.cat(samples).cpu().numpy()), _u32(y))
    assert one.carrier.sample == tx.carrier.sample == s0 + ref.NSYM * ref.SPS

    yref = o.tx_chain(ref.oracle_phasor(o, spec), bits, ref.SPS, None, w, s0, out_mode=o.OUT_IQ_BASEBAND)
    assert y.shape == yref.shape
    err = float(np.abs(y - yref).max())
    print(f"{name} s0={s0}: sample max|err| {err:.3g} (bound {1e-5 * float(np.abs(yref).max()):.3g})")
    assert err <= 1e-5 * np.abs(yref).max()


# ----------------------------------------------------------------- banks of channels ----
def _bank_spec(kind, c):
    """Channel c's phasor: parameters mixed within one kind (the batch's eligibility check only
    asks for one kind per bank)."""
    f = lambda v: float(np.float32(v))                                                       # noqa: E731
    if kind == "dmpsk":
        return ("dmpsk", 1 + c % 3, 1.0, f(0.1 + 0.37 * c), f(0.3 + 0.171 * c))
    if kind == "mfsk":
        return ("mfsk", 2 + c % 3, ((50, 120, 333)[(c // 6) % 3], 10000), 1.0, (c // 3) % 2)
    return ("bfsk", (100 + 7 * c, 10000), 1.0)


def _bank_lens(nch):
    """Symbols per channel for the two calls. Workgroup 0 (channels 0 .. 15) holds the edge counts
    0, 1, 63, 64, 65 and one channel of 1500 symbols among channels of fewer than 100 (its finished
    lanes idle through 22 more blocks); the second call swaps the longest and the empty channel."""
    n0 = [5 + (13 * c) % 90 for c in range(nch)]
    n0[:5] = [0, 1, 63, 64, 65]
    n0[7] = 1500
    n1 = [3 + (29 * c) % 95 for c in range(nch)]
    n1[0], n1[7] = 1500, 0
    return n0, n1


@functools.lru_cache(maxsize=None)
def bank_case(kind, nch):
    """Per channel: (spec, s0, bits of call 0, bits of call 1, symbols of call 0 and 1, oracle
    states over both calls, oracle samples over both calls); computed once, read-only."""
    import __graft_entry__ as graft
    o = graft.oracle()
    w = o.sample_freq(HZ, SR)
    n0, n1 = _bank_lens(nch)
    out = []
    for c in range(nch):
        spec = _bank_spec(kind, c)
        bps = ref.bps_of(spec)
        s0 = ref.S0S[c % 3] + 17 * c
        extra = c % bps if n1[c] > 0 else 0            # bits left over by call 0, taken up by call 1
        nb0 = bps * n0[c] + extra
        nb1 = bps * n1[c] - extra
        bits = o.prng_bits(ref.SEED + 0x100 + c, nb0 + nb1)
        states = ref.oracle_states(o, spec, bits, s0)
        assert len(states) == n0[c] + n1[c]
        y = o.tx_chain(ref.oracle_phasor(o, spec), bits, ref.SPS, None, w, s0, out_mode=o.OUT_IQ_BASEBAND)
        for a in (bits, states, y):
            a.setflags(write=False)
        out.append((spec, s0, bits[:nb0], bits[nb0:], n0[c], n1[c], states, y))
    return out


@pytest.mark.parametrize("nch", [17, 33])
@pytest.mark.parametrize("kind", ["dmpsk", "mfsk", "bfsk"])
def test_bank_states_bitwise(m, o, torch_cuda, kind, nch):
    """A bank whose last workgroup holds one channel (kScanCpw = 16: after 1 and after 2 full
    workgroups), with parameters mixed among the channels and ragged symbol counts, over two
    process_batch calls: after each call every channel's states are the oracle's for that channel
    (continuing from the first call), its samples are bitwise those of a handle of its own and
    within the sample tolerance of the oracle, and the carrier counters agree. Every channel
    reports that the bank launch (tx_scan_batch) computed its states."""
    torch = torch_cuda
    chans = bank_case(kind, nch)
    w = o.sample_freq(HZ, SR)
    bank = [_mod(m, w, s0, spec) for spec, s0, *_ in chans]
    singles = [_mod(m, w, s0, spec) for spec, s0, *_ in chans]
    # (a leftover bit after call 0 is in every bank whose symbols have more than one bit)
    assert kind == "bfsk" or any(len(ch[2]) % ref.bps_of(ch[0]) for ch in chans)
    pos = [0] * nch
    got_all = [[] for _ in range(nch)]
    for call in range(2):
        chunks = [torch.from_numpy(ch[2 + call].copy()).cuda() for ch in chans]
        got = m.DigitalModulator.process_batch(bank, chunks)
        for c, ch in enumerate(chans):
            spec, ns, want = ch[0], ch[4 + call], ch[6]
            cols = ref.COLUMNS[spec[0]]
            # the bank launch ran, not a quiet fall-back to one call per channel (the empty channel's
            # output has no address: the batch must take it all the same)
            assert bank[c].scan_path() == "bank", (c, call, bank[c].scan_path())
            st = bank[c].scan_states()
            assert st.shape == (ns, 2), (c, call, st.shape, ns)
            assert ref.same_bits(st, want[pos[c]:pos[c] + ns], cols), \
                (c, call, spec, ref.first_difference(st, want[pos[c]:pos[c] + ns], cols))
            single = singles[c].process(chunks[c])
            assert singles[c].scan_path() == "single"
            assert got[c].shape == single.shape == (ns * ref.SPS, 2), (c, call)
            assert np.array_equal(_u32(got[c].cpu().numpy()), _u32(single.cpu().numpy())), (c, call)
            assert bank[c].carrier.sample == singles[c].carrier.sample == ch[1] + (pos[c] + ns) * ref.SPS
            got_all[c].append(got[c])
            pos[c] += ns
    for c, ch in enumerate(chans):
        y, yref = torch.cat(got_all[c]).cpu().numpy(), ch[7]
        assert y.shape == yref.shape, c
        assert np.abs(y - yref).max() <= 1e-5 * np.abs(yref).max(), (c, ch[0], ch[1])


def test_scan_states_refusals(m, o, torch_cuda):
    """modem_tx_scan_states: UNSUPPORTED for a phasor without a scanned state, CAPACITY (with the
    count reported and the buffer untouched) when `cap` is one short, no states on a fresh handle."""
    torch = torch_cuda
    w = o.sample_freq(HZ, SR)
    qam = m.DigitalModulator(m.Carrier(w, 0), m.QAM(4, 0.0, 1.0), ref.SPS, None, out_mode=1)
    qam.process(torch.from_numpy(o.prng_bits(ref.SEED, 64)).cuda())
    with pytest.raises(m.ModemError) as e:
        qam.scan_states()
    assert e.value.status == m.ERR_UNSUPPORTED

    tx = _mod(m, w, 3, ref.KINDS["dqpsk"])
    fresh = tx.scan_states()
    assert fresh.shape == (0, 2) and fresh.dtype == np.float32
    assert tx.scan_path() == "none" and qam.scan_path() == "none"
    tx.process(torch.from_numpy(o.prng_bits(ref.SEED, 2 * 10)).cuda())
    L, sh = m.load_library(), m._stream_handle(None, 0)
    out = np.full((10, 2), 123.0, np.float32)
    n = ctypes.c_size_t(77)
    assert L.modem_tx_scan_states(tx._h, m._fptr(out), 9, ctypes.byref(n), sh) == m.ERR_CAPACITY
    assert n.value == 10 and np.all(out == 123.0)
    assert L.modem_tx_scan_states(tx._h, m._fptr(out), 10, ctypes.byref(n), sh) == m.MODEM_OK
    assert n.value == 10 and np.array_equal(_u32(out), _u32(tx.scan_states()))
