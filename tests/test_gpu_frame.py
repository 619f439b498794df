"""The frame synchronizer on the device against the restatement of tests/frame_ref.py: exact cases
(small-integer streams, every f32 sum exact: positions, counts and ok flags must be equal), noisy
float cases (proven free of borderline positions in tests/test_frame_host.py), streaming, the cap,
and the gather."""
import math

import numpy as np
import pytest

import frame_ref

pytestmark = pytest.mark.gpu

TURN_TOL = 2.0 ** -22


def _run(m, torch, x, u, W, thr, cuts=None, host=False, in_dtype=None, flush=True):
    """The stream x through process() at the given cut points, then flush(). Returns (pos, phi,
    metric) concatenated as numpy arrays and the list of per-call counts."""
    in_dtype = (m.DTYPE_F16 if x.dtype == np.float16 else m.DTYPE_F32) if in_dtype is None else in_dtype
    fs = m.FrameSync(u, guard=W, threshold=thr, in_dtype=in_dtype)
    xs = x if host else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    edges = [0] + list(cuts or []) + [len(x)]
    outs, counts = [], []
    calls = [fs.process(xs[a:b]) for a, b in zip(edges, edges[1:])]
    if flush:
        calls.append(fs.flush(like=None if host else xs))
    for pos, phi, met, cnt in calls:
        if not host:
            pos, phi, met, cnt = (t.cpu().numpy() for t in (pos, phi, met, cnt))
        c = int(cnt.view(np.uint64)[0])
        assert c <= len(pos)
        outs.append((pos.view(np.uint64)[:c].copy(), phi.view(np.uint32)[:c].copy(), met[:c].copy()))
        counts.append(c)
    assert fs.symbol == len(x)
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(3)), counts


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float64)
    return np.abs(a.astype(np.float64) - b) / np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)


def _check_exact(got, ref, what=""):
    pos, phi, met = got
    assert [int(p) for p in pos] == ref["pos"], what
    if len(pos):
        dt, du = frame_ref.turn_dist(phi, ref["turn"]).max(), _ulps(met, ref["metric"]).max()
        assert dt <= TURN_TOL and du <= 2, (what, dt, du)
        return dt / TURN_TOL, du / 2
    return 0.0, 0.0


def _ints(rng, n):
    return rng.randint(-1, 2, (n, 2)).astype(np.float32)


def _uw_ints(rng, L):
    return rng.choice([-1.0, 1.0], (L, 2)).astype(np.float32)


@pytest.mark.parametrize("L", [8, 9, 63, 256])
def test_exact_unique_words_around_every_tile_edge(m, torch_cuda, L):
    """W in {1, L, 256}; the unique word at stream index 0, at / one before / one after every
    multiple of 256 (the tile) up to 1024, the last one ending on the last symbol: found by the
    flush alone."""
    rng = np.random.RandomState(L)
    u = _uw_ints(rng, L)
    worst = (0.0, 0.0)
    for W in (1, L, 256):
        for d in (-1, 0, 1):
            n = 1024 + d + L
            x = _ints(rng, n)
            starts = [0] + [256 * k + d for k in (1, 2, 3, 4)]
            for s in starts:
                x[s:s + L] = u
            ref = frame_ref.detect(x, u, W, 0.9)
            got, counts = _run(m, torch_cuda, x, u, W, 0.9)
            worst = tuple(max(a, b) for a, b in zip(worst, _check_exact(got, ref, (L, W, d))))
            assert sum(counts) == len(ref["pos"])
            assert counts[0] == sum(p < frame_ref.decided(n, W, L) for p in ref["pos"])
            if W < 256:                                                 # (at W = 256 the words are rivals: equal maxima)
                assert ref["pos"][0] == 0 and ref["pos"][-1] == starts[-1] and counts[1] >= 1   # the last one needs the flush
    print(f"L {L}: worst phi error / bound {worst[0]:.3f}, worst metric error / bound {worst[1]:.3f}")


def test_exact_two_words_a_guard_apart(m, torch_cuda):
    """Two unique words W apart give one hit (equal maxima, the earliest wins), W + 1 apart two."""
    rng = np.random.RandomState(2)
    L, W = 8, 12
    u = _uw_ints(rng, L)
    x = np.zeros((600, 2), np.float32)
    for s in (100, 100 + W, 300, 300 + W + 1):
        x[s:s + L] = u
    ref = frame_ref.detect(x, u, W, 0.9)
    assert ref["pos"] == [100, 300, 300 + W + 1]
    got, _ = _run(m, torch_cuda, x, u, W, 0.9)
    _check_exact(got, ref)


def test_exact_back_to_back_words_the_earliest_wins(m, torch_cuda):
    rng = np.random.RandomState(3)
    u = _uw_ints(rng, 8)
    x = np.zeros((700, 2), np.float32)
    x[250:250 + 40] = np.tile(u, (5, 1))                               # equal maxima across a tile edge
    ref = frame_ref.detect(x, u, 8, 0.9)
    assert ref["pos"] == [250]
    got, _ = _run(m, torch_cuda, x, u, 8, 0.9)
    _check_exact(got, ref)


def test_exact_degenerate_streams(m, torch_cuda):
    """All zeros: no hit. Shorter than L: nothing to decide. Exactly L symbols: found by the flush."""
    rng = np.random.RandomState(4)
    u = _uw_ints(rng, 16)
    got, counts = _run(m, torch_cuda, np.zeros((1000, 2), np.float32), u, 16, 0.5)
    assert len(got[0]) == 0 and counts == [0, 0]
    got, counts = _run(m, torch_cuda, u[:15].copy(), u, 16, 0.5)
    assert counts == [0, 0]
    got, counts = _run(m, torch_cuda, u.copy(), u, 16, 0.5)
    assert counts == [0, 1] and int(got[0][0]) == 0 and got[2][0] == 1.0
    got, counts = _run(m, torch_cuda, np.zeros((0, 2), np.float32), u, 16, 0.5)
    assert counts == [0, 0]


def test_exact_nan_and_inf_inside_and_beside_a_word(m, torch_cuda):
    """A non-finite symbol makes every position whose window holds it non-finite: no candidate, and
    no condition on its neighbours."""
    rng = np.random.RandomState(6)
    L, W = 16, 16
    u = _uw_ints(rng, L)
    x = _ints(rng, 900)
    for s in (100, 300, 500, 700):
        x[s:s + L] = u
    x[105, 0] = np.nan                                                 # inside: the word at 100 is lost
    x[299, 1] = np.inf                                                 # just before the word at 300: it stays
    x[516, 0] = -np.inf                                                # just after the word at 500: it stays
    x[707, 1] = np.inf                                                 # inside
    ref = frame_ref.detect(x, u, W, 0.9)
    assert ref["pos"] == [300, 500]
    got, _ = _run(m, torch_cuda, x, u, W, 0.9)
    _check_exact(got, ref)


@pytest.mark.parametrize("name", list(frame_ref.NOISY))
def test_noisy_cases_give_the_restatements_hits(m, torch_cuda, name):
    x, u = frame_ref.noisy_case(m, name)
    ref = frame_ref.detect(x, u, len(u), frame_ref.NOISY_THR)
    assert ref["borderline"] == []
    (pos, phi, met), _ = _run(m, torch_cuda, x, u, len(u), frame_ref.NOISY_THR)
    assert [int(p) for p in pos] == ref["pos"] == list(frame_ref.NOISY_STARTS)
    worst_m = worst_p = 0.0
    for i, k in enumerate(ref["pos"]):
        bound = frame_ref.metric_bound(ref, k)
        tol = TURN_TOL + ref["dm"][k] / ref["m"][k] / (4 * math.pi)     # the angle of c moves by <= |dc| / |c| radians
        dm, dp = abs(float(met[i]) - ref["metric"][i]), float(frame_ref.turn_dist(phi[i:i + 1], ref["turn"][i:i + 1])[0])
        worst_m, worst_p = max(worst_m, dm / bound), max(worst_p, dp / tol)
        assert dm <= bound and dp <= tol, (k, dm, bound, dp, tol)
    print(f"{name}: worst metric error / bound {worst_m:.3f}, worst phi error / bound {worst_p:.3f}")


@pytest.fixture(scope="module")
def stream_case(m):
    """About 3000 noisy symbols with five unique words, one across the end of the stream's decided part."""
    x, u = frame_ref.noisy_case(m, "qpsk-32-f32")
    x = np.concatenate([x, x[:1490]])
    return x, u, frame_ref.detect(x, u, 32, 0.6)


def test_any_cut_of_a_stream_gives_the_same_hits(m, torch_cuda, stream_case):
    x, u, ref = stream_case
    n = len(x)
    one, _ = _run(m, torch_cuda, x, u, 32, 0.6)
    assert [int(p) for p in one[0]] == ref["pos"] and len(ref["pos"]) == 6
    primes = list(np.cumsum([7, 13, 101, 257, 499, 997, 2, 3, 61]))
    zeros = sorted([0, 0, 700, 700, 700, 1500, n, n])
    for cuts in (list(range(1, n)), primes, zeros):
        got, _ = _run(m, torch_cuda, x, u, 32, 0.6, cuts=cuts)
        for a, b in zip(one, got):
            assert a.tobytes() == b.tobytes()


def test_host_pointers_and_offset_views(m, torch_cuda, stream_case):
    x, u, _ = stream_case
    torch = torch_cuda
    one, _ = _run(m, torch, x, u, 32, 0.6)
    host, _ = _run(m, torch, x, u, 32, 0.6, host=True, cuts=[1000])
    for a, b in zip(one, host):
        assert a.tobytes() == b.tobytes()
    for half in (False, True):
        xs = x.astype(np.float16) if half else x
        want, _ = _run(m, torch, xs, u, 32, 0.6)
        buf = torch.zeros(2 * len(x) + 4, dtype=torch.float16 if half else torch.float32, device="cuda")
        for off in (2, 1):                                             # one symbol, one element into the buffer
            v = buf[off:off + 2 * len(x)].view(-1, 2)
            v.copy_(torch.from_numpy(xs).cuda())
            fs = m.FrameSync(u, guard=32, threshold=0.6, in_dtype=m.DTYPE_F16 if half else m.DTYPE_F32)
            a = fs.process(v[:1234])
            b = fs.process(v[1234:])
            c = fs.flush(like=v)
            pos = np.concatenate([t[0].cpu().numpy()[:int(t[3][0])] for t in (a, b, c)]).view(np.uint64)
            met = np.concatenate([t[2].cpu().numpy()[:int(t[3][0])] for t in (a, b, c)])
            assert pos.tobytes() == want[0].tobytes() and met.tobytes() == want[2].tobytes()


def test_a_small_cap_keeps_the_count_and_writes_nothing_past_it(m, torch_cuda, stream_case):
    x, u, ref = stream_case
    torch = torch_cuda
    L = m.load_library()
    xs = torch.from_numpy(x).cuda()
    full = m.FrameSync(u, guard=32, threshold=0.6)
    want = full.process(xs)
    nwant = int(want[3][0])
    assert nwant >= 4
    fs = m.FrameSync(u, guard=32, threshold=0.6)
    pos = torch.full((8,), -7, dtype=torch.int64, device="cuda")
    phi = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    met = torch.full((8,), -7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    st = L.modem_frame_process(fs._h, xs.data_ptr(), len(x), pos.data_ptr(), phi.data_ptr(), met.data_ptr(), 2, cnt.data_ptr(), None)
    assert st == m.MODEM_OK
    assert int(cnt[0]) == nwant                                        # never capped
    assert torch.equal(pos[:2], want[0][:2]) and torch.equal(phi[:2], want[1][:2]) and torch.equal(met[:2], want[2][:2])
    assert bool((pos[2:] == -7).all()) and bool((phi[2:] == -7).all()) and bool((met[2:] == -7.0).all())
    fs._ncarry = full._ncarry
    a, b = fs.process(xs[:600]), full.process(xs[:600])                # the state advanced as with a large cap
    na = int(a[3][0])
    assert na == int(b[3][0]) == 2 and torch.equal(a[0][:na], b[0][:na]) and torch.equal(a[2][:na], b[2][:na])
    assert int(a[0][0]) == len(x) + ref["pos"][0]
    hp, hc = np.full(8, 99, np.uint64), np.zeros(1, np.uint64)         # host outputs: the same rule
    fs2 = m.FrameSync(u, guard=32, threshold=0.6)
    st = L.modem_frame_process(fs2._h, x.ctypes.data, len(x), hp.ctypes.data, None, None, 1, hc.ctypes.data, None)
    assert st == m.MODEM_OK and int(hc[0]) == nwant and int(hp[0]) == ref["pos"][0] and (hp[1:] == 99).all()


# ------------------------------------------------------------------------------ gather ----
def _quarter(z, q):
    """z (-j)^q by swaps and sign changes."""
    return [z, z.imag - 1j * z.real, -z, -z.imag + 1j * z.real][q % 4]


def _gather(m, torch, x, base, pos, phi, count, host=False, **kw):
    fs = m.FrameSync(np.ones((8, 2), np.float32), in_dtype=m.DTYPE_F16 if x.dtype == np.float16 else m.DTYPE_F32)
    pos = np.asarray(pos, np.uint64)
    phi = None if phi is None else np.asarray(phi, np.uint32)
    cnt = np.array([count], np.uint64)
    if host:
        fr, ok = fs.gather(x, base, pos, phi, cnt, **kw)
        return np.asarray(fr, np.float64), ok
    dev = lambda a, dt: None if a is None else torch.from_numpy(a.view(dt)).cuda()
    fr, ok = fs.gather(torch.from_numpy(x).cuda(), base, dev(pos, np.int64), dev(phi, np.int32), dev(cnt, np.int64), **kw)
    return fr.cpu().numpy().astype(np.float64), ok.cpu().numpy()


@pytest.mark.parametrize("power", [1, 2, 4, 8])
def test_gather_rotations(m, torch_cuda, power):
    """Every rot of M = 1, 2, 4 exactly; M = 8 within 2^-20 |r| of the float64 rotation. Odd length
    and odd positions (unaligned rows), base != 0, a row cut by either end, rows past count."""
    rng = np.random.RandomState(power)
    x = rng.standard_normal((400, 2)).astype(np.float32)
    base, length, skip = 1000, 37, 5
    phis = sorted({(r * ((1 << 32) // power) + d) & 0xFFFFFFFF for r in range(power) for d in (0, -(1 << 28) // power, (1 << 28) // power)}) if power > 1 else [0, 1 << 31]
    pos = [base + 3 + 7 * i for i in range(len(phis))] + [base - 6, base + 400 - skip - length + 1, base + 20, base + 21]
    phi = phis + [0, 0, 1 << 30, 1 << 30]
    count = len(phis) + 3                                               # the last row lies past count
    fr, ok = _gather(m, torch_cuda, x, base, pos, phi, count, skip=skip, length=length, power=power)
    want_ok = [1] * len(phis) + [0, 0, 1, 0]
    assert ok.tolist() == want_ok
    z, got = frame_ref.cplx(x), fr[..., 0] + 1j * fr[..., 1]
    worst = 0.0
    for f in range(len(pos)):
        if not want_ok[f]:
            assert not fr[f].any()
            continue
        a = pos[f] + skip - base
        rot = frame_ref.rot_of(phi[f], power)
        if power <= 4 or rot % 2 == 0:
            assert np.array_equal(got[f], _quarter(z[a:a + length], rot * 4 // power if power > 1 else 0))
        else:
            want = z[a:a + length] * np.exp(-2j * np.pi * rot / 8)
            err = np.abs(got[f] - want) / np.abs(z[a:a + length])
            worst = max(worst, float(err.max()) / 2.0 ** -20)
            assert err.max() <= 2.0 ** -20
    assert sorted({frame_ref.rot_of(p, power) for p in phis}) == list(range(power))
    if power == 8:
        print(f"M = 8: worst rotation error / bound {worst:.3f}")


def test_gather_f16_host_and_no_rotation(m, torch_cuda):
    """F16 in and out (M = 8: the f16 storage term on top), phi = None, host pointers, aligned rows."""
    rng = np.random.RandomState(9)
    x16 = rng.standard_normal((300, 2)).astype(np.float16)
    pos, phi = [0, 16, 101, 250], [3 << 29, 1 << 29, 5 << 29, 0]
    z = frame_ref.cplx(x16)
    for host in (False, True):
        fr, ok = _gather(m, torch_cuda, x16, 0, pos, phi, 4, host=host, skip=0, length=64, power=8, out_dtype=m.DTYPE_F16)
        assert ok.tolist() == [1, 1, 1, 0]
        got = fr[..., 0] + 1j * fr[..., 1]
        for f in range(3):
            r = z[pos[f]:pos[f] + 64]
            want = r * np.exp(-2j * np.pi * frame_ref.rot_of(phi[f], 8) / 8)
            tol = 2.0 ** -20 * np.abs(r) + math.sqrt(2.0) * np.maximum(2.0 ** -11 * np.abs(r), 2.0 ** -25)   # f16: half an ulp per component
            assert (np.abs(got[f] - want) <= tol).all()
        fr, ok = _gather(m, torch_cuda, x16, 0, pos, None, 4, host=host, skip=0, length=64, power=8)
        assert ok.tolist() == [1, 1, 1, 0] and not fr[3].any()
        for f in range(3):
            assert np.array_equal(fr[f, :, 0] + 1j * fr[f, :, 1], z[pos[f]:pos[f] + 64])
