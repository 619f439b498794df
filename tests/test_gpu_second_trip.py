"""Every capped-grid stage at the smallest size where its loops take a second trip.

The demapper, the differential detector, the channel, the error counter, the three synchronizers
and the encoder launch at most 2048 workgroups and cover the rest in a grid-stride loop; the
synchronizers' one-workgroup prefix scans take 1024 items per round. The other GPU tests stay below
every one of those thresholds, so the loop increments, the carried scan base and the per-trip phase
and counter steps run here for the first time under a test that looks at the output. Every size in
SIZES crosses its threshold by a non-round amount (the last trip is partial), and
tests/test_second_trip_sizes.py recomputes the thresholds from the kernels' own constants and fails
if one of these sizes no longer crosses.

Each case is held against the restatement, the bounds and the check helpers of the kernel's own
small-shape test file; integer outputs (theta, D, positions, counts, coded bits, error counts) are
exact. The synchronizers use the vectorised restatements, which the host tests hold equal to the
per-block ones. frame_emit_kernel's grid-stride trip (more than 524,288 tiles) is the one second
trip left uncovered."""
import numpy as np
import pytest

import chan_ref
import fec_ref
import frame_ref
import timing_ref as R
import test_gpu_chan as C
import test_gpu_demap as DM
import test_gpu_diff as DF
import test_gpu_fec as FE
import test_gpu_frame as FR
import test_gpu_sync as SY
import test_gpu_timing as TM

pytestmark = pytest.mark.gpu

# What each case feeds its kernel. tests/test_second_trip_sizes.py holds every entry above the
# threshold read from the .hip sources.
SIZES = {
    "sync": dict(block=64, nsym=(32768 + 9) * 64 + 17),                  # 33 scan rounds, 5 estimator trips, 2 apply trips
    "timing": dict(sps=4, block=32, nsamp=(65536 + 9) * 32 * 4 + 17 * 4 + 3),
    "frame": dict(L=8, W=8, nsym=1027 * 256 + 37 + 8 + 8 - 1),           # 1027 * 256 + 37 decided positions: 1028 tiles
    "gather": dict(cap=2048 + 5),
    "chan": dict(n=2097152 + 4 * 256 * 3 + 3),
    "count_aligned": dict(n=16 * 524288 + 16 * 300 + 7),
    "count_bytewise": dict(n=524288 + 1000 + 3),
    "count_common": dict(n=16 * 524288 + 16 * 300 + 7, skew=5),
    "demap": dict(nsym=524288 + 256 * 3 + 5),
    "diff": dict(nsym=524288 + 256 * 3 + 5),
    "encode_k3": dict(K=3, polys=(7, 5), nbits=62, nframes=8200),
    "encode_k7": dict(K=7, polys=(0o171, 0o133, 0o165), nbits=58, nframes=8200),
}
MAX_CALL_BLOCKS = 1024          # calls of at most this many blocks use only what the small-shape tests cover


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _cat_bytes(torch, parts):
    return _bytes(torch.cat(list(parts)))


# ------------------------------------------------------------------ carrier synchronizer ----
def _sync_stream(m):
    return SY.stream(m, "bpsk", SIZES["sync"]["block"], SIZES["sync"]["nsym"])


def _sync_calls(m, torch, xin, dtype, edges):
    """The stream through one handle in the calls `edges` delimit, then flush: the bytes of
    (out, theta, q, flush) over the whole stream and the handle's symbol count."""
    sy = SY.make_sync(m, "bpsk", SIZES["sync"]["block"], in_dtype=dtype, out_dtype=dtype)
    x = torch.from_numpy(xin).cuda()
    calls = [sy.process(x[a:b]) for a, b in zip(edges, edges[1:])]
    rest = sy.flush(like=x)
    assert sy.symbol == len(xin)
    return tuple(_cat_bytes(torch, (c[i] for c in calls)) for i in range(3)) + (_bytes(rest),)


def _short_cuts(n, per_call):
    return list(range(0, n, per_call)) + [n]


@pytest.mark.parametrize("dtype", [0, 1])
def test_carrier_sync_against_the_restatement(m, torch_cuda, dtype):
    """q_b >= 0.3 and margins >= 0.1 turn are asserted by run_parity; theta is exact."""
    want, th, got, xin = SY.run_parity(m, torch_cuda, "bpsk", dtype, dtype, fast=True, **SIZES["sync"])
    nb = SIZES["sync"]["nsym"] // 64
    assert len(th) == nb == 32777 and len(got) == SIZES["sync"]["nsym"]
    assert nb > 32 * MAX_CALL_BLOCKS and nb > 4 * 8192 and nb * 64 > 2097152


@pytest.mark.parametrize("dtype", [0, 1])
def test_carrier_sync_one_call_equals_short_calls(m, torch_cuda, dtype):
    """The header's cut invariance: calls of at most 1001 blocks each (a carry in between) use only
    the first trip of every loop."""
    x32, _, block = _sync_stream(m)
    xin = x32.astype(SY.NP_DT[dtype])
    per = 1000 * block + 13
    assert (per + block - 1) // block <= MAX_CALL_BLOCKS
    one = _sync_calls(m, torch_cuda, xin, dtype, [0, len(xin)])
    cut = _sync_calls(m, torch_cuda, xin, dtype, _short_cuts(len(xin), per))
    assert one == cut


def test_carrier_sync_workspace_growth(m, torch_cuda):
    """A small call, the large call, a small call on one handle: the workspace grows in the second
    call, with a carry and a scan state alive. The handle advances as over one contiguous stream:
    the same bytes as the whole stream in one call on a fresh handle (which grows before it holds
    any state) and as short calls (which never outgrow their first buffers by much)."""
    x32, _, block = _sync_stream(m)
    xin = np.array(x32)
    n = len(xin)
    grown = _sync_calls(m, torch_cuda, xin, 0, [0, 3 * block + 5, n - 2 * block - 3, n])
    assert grown == _sync_calls(m, torch_cuda, xin, 0, [0, n])
    assert grown == _sync_calls(m, torch_cuda, xin, 0, _short_cuts(n, 1000 * block + 13))


# ------------------------------------------------------------------- timing synchronizer ----
TIMING_BETA, TIMING_DRIFT_TOTAL, TIMING_REACH = 1.0, 1.5, 3
_TIMING = {}


def _timing_stream():
    """timing_ref's generator at 65,545 blocks of 32 symbols, sps 4: the small cases' delay, noise and
    tracker start, but roll-off 1.0 (at 0.5 the restatement's q_b falls to 0.002 somewhere in 65,545
    blocks of 32 symbols; at 1.0 its minimum is 0.025 and the smallest margin 0.38 symbol), a drift
    of 1.5 symbols over the whole stream (the delay stays inside the span of 2, and Phi wraps
    once), and the pulse cut at +-3 symbols to keep the generator to a few seconds."""
    if not _TIMING:
        sps, block, n = (SIZES["timing"][k] for k in ("sps", "block", "nsamp"))
        rng = np.random.RandomState(sps * 1000 + block)
        nsym = n // sps + 2
        pts = ((2 * rng.randint(0, 2, nsym) - 1) + 1j * (2 * rng.randint(0, 2, nsym) - 1)) / np.sqrt(2)
        z = R.stream(pts, sps, n, R.CASE_TAU, TIMING_DRIFT_TOTAL / (n / sps), TIMING_BETA, reach=TIMING_REACH)
        sig = np.sqrt(1.0 / (2 * 10.0 ** (R.CASE_EBN0_DB / 10)) / 2)
        z = z + sig * (rng.randn(n) + 1j * rng.randn(n))
        x = R.pairs(z).astype(np.float32)
        x.setflags(write=False)
        _TIMING["x"] = x
    return _TIMING["x"], SIZES["timing"]["sps"], SIZES["timing"]["block"]


def _timing_calls(m, torch, xin, dtype, edges):
    sps, block = SIZES["timing"]["sps"], SIZES["timing"]["block"]
    ts = m.TimingSync(sps, block=block, span=R.CASE_SPAN, tau0=R.CASE_TAU0, in_dtype=dtype, out_dtype=dtype)
    x = torch.from_numpy(xin).cuda()
    calls = [ts.process(x[a:b]) for a, b in zip(edges, edges[1:])]
    rest = ts.flush(like=x)
    assert ts.sample == len(xin)
    return tuple(_cat_bytes(torch, (c[i] for c in calls)) for i in range(3)) + (_bytes(rest),)


@pytest.mark.parametrize("in_dtype", [0, 1])
def test_timing_sync_against_the_restatement(m, torch_cuda, in_dtype):
    """q_b >= 0.02 and margins >= 0.1 symbol are asserted by run_parity; D is exact; every output
    symbol is compared in float64 (no restriction to a subset of the blocks)."""
    x, sps, block = _timing_stream()
    want, D, got = TM.run_parity(m, torch_cuda, "second-trip", in_dtype, 0, case=(x, sps, block), fast=True)
    nb = len(x) // (block * sps)
    assert len(D) == nb == 65545 and len(got) == nb * block + 17
    assert nb > 64 * MAX_CALL_BLOCKS and nb > 8 * 8192 and nb * block > 2097152
    assert max(abs(d) for d in D) < R.CASE_SPAN << 32                       # the clamp stays out of it
    assert max(D) - min(D) > 1 << 32                                        # and Phi wrapped


@pytest.mark.parametrize("dtype", [0, 1])
def test_timing_sync_one_call_equals_short_calls(m, torch_cuda, dtype):
    x32, sps, block = _timing_stream()
    xin = x32.astype(TM.NP_DT[dtype])
    per = 1000 * block * sps + 7 * sps + 1
    assert (per + block * sps - 1) // (block * sps) <= MAX_CALL_BLOCKS
    one = _timing_calls(m, torch_cuda, xin, dtype, [0, len(xin)])
    cut = _timing_calls(m, torch_cuda, xin, dtype, _short_cuts(len(xin), per))
    assert one == cut


def test_timing_sync_workspace_growth(m, torch_cuda):
    """As test_carrier_sync_workspace_growth."""
    x32, sps, block = _timing_stream()
    xin = np.array(x32)
    n, bn = len(xin), block * sps
    grown = _timing_calls(m, torch_cuda, xin, 0, [0, 3 * bn + 5, n - 2 * bn - 3, n])
    assert grown == _timing_calls(m, torch_cuda, xin, 0, [0, n])
    assert grown == _timing_calls(m, torch_cuda, xin, 0, _short_cuts(n, 1000 * bn + 7 * sps + 1))


# -------------------------------------------------------------------- frame synchronizer ----
def _frame_stream(d):
    """Small integers (every f32 sum exact), the unique word at index 0, inside tile 511, at
    1023 * 256 + d and 1024 * 256 + d (either side of the scan's round edge), in the last tile and
    on the last L symbols (found by the flush alone); background everywhere else."""
    L, W, n = (SIZES["frame"][k] for k in ("L", "W", "nsym"))
    rng = np.random.RandomState(100 + d)
    u = FR._uw_ints(rng, L)
    x = FR._ints(rng, n)
    starts = [0, 511 * 256 + 100, 1023 * 256 + d, 1024 * 256 + d, 1027 * 256 + 10, n - L]
    for s in starts:
        x[s:s + L] = u
    return x, u, starts


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_frame_sync_hits_on_either_side_of_the_round_edge(m, torch_cuda, d):
    """Positions, per-call counts and the flush count equal frame_ref.detect; phi and the metric
    within _check_exact's bounds. The restatement reports no borderline position (asserted)."""
    L, W, n = (SIZES["frame"][k] for k in ("L", "W", "nsym"))
    x, u, starts = _frame_stream(d)
    ref = frame_ref.detect(x, u, W, 0.9)
    assert set(starts) <= set(ref["pos"]) and ref["borderline"] == []
    decided = frame_ref.decided(n, W, L)
    assert (decided + 255) // 256 == 1028 and decided % 256
    got, counts = FR._run(m, torch_cuda, x, u, W, 0.9)
    FR._check_exact(got, ref, d)
    assert counts == [sum(p < decided for p in ref["pos"]), sum(p >= decided for p in ref["pos"])]
    assert counts[1] >= 1
    edge = 1024 * 256
    below, above = [p for p in ref["pos"] if p < edge], [p for p in ref["pos"] if p >= edge]
    assert len(below) >= 3 and len(above) >= 2                           # a lost base moves the later hits' slots


def test_frame_sync_workspace_growth(m, torch_cuda):
    """A small call, the large call, a small call on one handle, then the flush: the hits of the
    whole stream in one call, and of frame_ref.detect."""
    L, W, n = (SIZES["frame"][k] for k in ("L", "W", "nsym"))
    x, u, _ = _frame_stream(0)
    ref = frame_ref.detect(x, u, W, 0.9)
    one, _ = FR._run(m, torch_cuda, x, u, W, 0.9)
    got, counts = FR._run(m, torch_cuda, x, u, W, 0.9, cuts=[700, n - 900])
    FR._check_exact(got, ref)
    assert len(counts) == 4 and sum(counts) == len(ref["pos"])
    for a, b in zip(one, got):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------ gather ----
def test_frame_gather_more_rows_than_workgroups(m, torch_cuda):
    """cap = 2053 rows of 5 symbols (unaligned rows), count = cap - 2, power 4 with phi cycling
    through the four quarter turns; some positions cut by either end of the 400-symbol input."""
    cap = SIZES["gather"]["cap"]
    count, length, skip, base, nin = cap - 2, 5, 3, 1000, 400
    rng = np.random.RandomState(cap)
    x = rng.standard_normal((nin, 2)).astype(np.float32)
    room = nin - skip - length + 1                                      # rows that fit start at 0 .. room - 1 after the skip
    pos = [base + (7 * f) % room for f in range(cap)]
    for f, p in ((3, base - skip - 1), (100, base - 4), (2047, base + room), (2049, base + room + 5), (2050, base - 9)):
        pos[f] = p
    phi = [(f % 4) << 30 for f in range(cap)]
    fr, ok = FR._gather(m, torch_cuda, x, base, pos, phi, count, skip=skip, length=length, power=4)
    assert fr.shape == (cap, length, 2) and ok.shape == (cap,)
    z, got = frame_ref.cplx(x), fr[..., 0] + 1j * fr[..., 1]
    want_ok = []
    for f in range(cap):
        a = pos[f] + skip - base
        valid = f < count and a >= 0 and a + length <= nin
        want_ok.append(int(valid))
        if valid:
            assert frame_ref.rot_of(phi[f], 4) == f % 4
            assert np.array_equal(got[f], FR._quarter(z[a:a + length], f % 4)), f
        else:
            assert not fr[f].any(), f
    assert ok.tolist() == want_ok
    assert want_ok[2048] == 1 and want_ok[2049] == 0 and want_ok[2050] == 0 and want_ok[cap - 1] == 0 and want_ok[cap - 2] == 0
    assert sum(want_ok) == count - 5


# ----------------------------------------------------------------------------- channel ----
_CHAN = {}
CHAN_S0 = (1 << 40) + 3


def _chan_scatter():
    if not _CHAN:
        rng = np.random.RandomState(20241)
        x = (rng.randn(SIZES["chan"]["n"], 2) * np.sqrt(0.5)).astype(np.float32)
        x[[0, 5, 2097151, 2097153]] *= np.float32(1e-3)
        x[[2, 66, 2097152, len(x) - 1]] *= np.float32(1e3)
        x.setflags(write=False)
        _CHAN["x"] = x
    return _CHAN["x"]


@pytest.mark.parametrize("case,dtype", [("both", 0), ("both", 1), ("noise", 0), ("rot", 0)])
def test_channel_against_the_restatement(m, torch_cuda, case, dtype):
    """`both` as f32 -> f32 and f16 -> f16; noise alone and rotation alone, so that the per-trip
    steps of the noise counter and of the NCO phase are each held on their own."""
    C.run_parity(m, torch_cuda, _chan_scatter(), C.CASES[case], CHAN_S0, dtype, dtype,
                 f"{case} second trip {'f16' if dtype else 'f32'}", rotate=chan_ref.rotate_np)


@pytest.mark.parametrize("dtype", [0, 1])
def test_channel_one_call_equals_two_calls(m, torch_cuda, dtype):
    torch = torch_cuda
    kw = dict(C.CASES["both"], s0=CHAN_S0, in_dtype=dtype, out_dtype=dtype)
    x = torch.from_numpy(_chan_scatter().astype(C.NP_DT[dtype])).cuda()
    whole = m.Channel(**kw).process(x)
    cut, at = m.Channel(**kw), 1048577
    parts = [cut.process(x[:at]), cut.process(x[at:])]
    assert cut.sample == CHAN_S0 + len(x)
    assert _cat_bytes(torch, parts) == _bytes(whole)


# ------------------------------------------------------------------------ error counter ----
def _error_pattern(n, seed):
    """Random bytes, about 1 % of them differing (by 1 to 8 bits)."""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, n).astype(np.uint8)
    flip = np.where(rng.rand(n) < 0.01, rng.randint(1, 256, n), 0).astype(np.uint8)
    flip[-1] = 0x81
    return a, a ^ flip


@pytest.mark.parametrize("name,oa,ob", [("count_aligned", 0, 0), ("count_bytewise", 0, 1), ("count_common", 5, 5)])
def test_count_errors_past_the_grid(m, torch_cuda, name, oa, ob):
    """Both pointers 16-byte aligned; b one byte into its allocation (no common boundary: the
    bytewise path for all n); both 5 bytes in (a head of 11 bytes, then vectors, then a tail)."""
    torch = torch_cuda
    n = SIZES[name]["n"]
    a, b = _error_pattern(n, n % 1000)
    x = a ^ b
    want = [int(np.count_nonzero(x)), int(np.unpackbits(x).sum())]
    assert 0.005 * n < want[0] < 0.02 * n
    da, db = torch.zeros(n + 16, dtype=torch.uint8, device="cuda"), torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    assert da.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0
    va, vb = da[oa:oa + n], db[ob:ob + n]
    va.copy_(torch.from_numpy(a))
    vb.copy_(torch.from_numpy(b))
    c = m.count_errors(va, vb)
    assert c.tolist() == want
    m.count_errors(va, vb, counts=c)                                    # accumulates
    assert c.tolist() == [2 * want[0], 2 * want[1]]


# --------------------------------------------------- demapper and differential detector ----
@pytest.mark.parametrize("name,out", [("qam16", "i8"), ("mpsk8", "f16")])
def test_demapper_past_the_grid(m, torch_cuda, name, out):
    """The axis-separable path with int8 output (scale 256: clipping on both sides) and the point
    table with f16 output (no value near the f16 range: the in-range rule everywhere)."""
    torch = torch_cuda
    n = SIZES["demap"]["nsym"]
    scale = DM.I8_SCALE if out == "i8" else DM.SCALES[name]
    iq = DM.scatter(name, n, seed=3)
    ref, bound = DM.ref_llr(DM._lut_of(name), iq, scale)
    dm = DM._demapper(m, name, out_dtype=m.DTYPE_I8 if out == "i8" else m.DTYPE_F16)
    assert dm.path == DM.CONSTELLATIONS[name][3]
    got = dm.process(torch.from_numpy(iq).cuda(), scale)
    assert tuple(got.shape) == ref.shape
    g = got.cpu().numpy().astype(np.float64)
    if out == "i8":
        assert got.dtype == torch.int8
        DM._check_i8(g, ref, bound)
    else:
        assert got.dtype == torch.float16
        sat, inside = DM._check_f16(g, ref, bound)
        assert inside.all()


def test_diff_detector_past_the_grid(m, torch_cuda):
    torch = torch_cuda
    n, bps = SIZES["diff"]["nsym"], 2
    _, iq = DF.synth(bps, n, 0.15)
    _, rsym, rllr, bound, margin, P = DF.ref_diff(DF._lut_of(bps), iq, DF.prev0_of(), DF.SCALES[bps])
    sym, llr = DF.phasor(m, bps).detector().process(torch.from_numpy(iq).cuda(), DF.SCALES[bps])
    assert sym.dtype == torch.uint8 and llr.dtype == torch.float32 and tuple(llr.shape) == (n, bps)
    DF._check_f32(llr.cpu().numpy(), rllr, bound, "dqpsk second trip")
    DF._check_sym(sym.cpu().numpy(), rsym, margin, P, "dqpsk second trip")


# ----------------------------------------------------------------------------- encoder ----
@pytest.mark.parametrize("name", ["encode_k3", "encode_k7"])
def test_encoder_past_the_grid(m, torch_cuda, name):
    """Input rows 3 bytes longer than nbits, bytes with high bits set, output rows followed by 5
    sentinel bytes (checked by _encode_raw)."""
    K, polys, nbits, nframes = (SIZES[name][k] for k in ("K", "polys", "nbits", "nframes"))
    rng = np.random.RandomState(K)
    bits = rng.randint(0, 256, (nframes, nbits + 3)).astype(np.uint8)
    got = FE._encode_raw(m, torch_cuda, m.ConvCode(K, polys), bits, nbits, pad=5)
    assert np.array_equal(got, fec_ref.encode(bits[:, :nbits], K, polys))
