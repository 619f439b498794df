"""The sizes of tests/test_gpu_second_trip.py against the kernels' own constants (no device needed).

A test cannot observe gridDim. This one reads the launch caps, the workgroup sizes, the per-lane
group sizes and the scan widths out of the .hip sources, recomputes the size at which each loop
takes its second trip, and asserts that every size the GPU tests use lies above it. Raising a cap
makes this test fail instead of the coverage vanishing."""
import os
import re

from conftest import ROOT
import test_gpu_second_trip as T

CSRC = os.path.join(ROOT, "rust-modem_amd", "csrc")


def _consts(fname):
    """Every `constexpr int kName = <integer>` of a source file."""
    with open(os.path.join(CSRC, fname)) as f:
        text = f.read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (k\w+) = (\d+)\s*[;,]", text)}, text


def test_every_size_crosses_its_threshold():
    S = T.SIZES
    c, _ = _consts("modem_sync.hip")
    nb = S["sync"]["nsym"] // S["sync"]["block"]
    assert nb > c["kScanPer"] * c["kSyncNT"]                                   # sync_scan_kernel: a second round
    assert nb > 32 * c["kScanPer"] * c["kSyncNT"]
    assert nb > c["kSyncMaxBlocks"] * (c["kSyncNT"] // 64)                     # sync_est_kernel
    assert nb * S["sync"]["block"] > c["kSyncMaxBlocks"] * c["kSyncNT"] * c["kSyncG"]      # sync_apply_kernel
    assert S["sync"]["nsym"] % S["sync"]["block"]                               # and a flush
    assert T.MAX_CALL_BLOCKS <= c["kScanPer"] * c["kSyncNT"]                    # the short calls stay in the first round

    c, _ = _consts("modem_timing.hip")
    nb = S["timing"]["nsamp"] // (S["timing"]["block"] * S["timing"]["sps"])
    assert nb > c["kTimScanPer"] * c["kTimNT"]
    assert nb > c["kTimMaxBlocks"] * (c["kTimNT"] // 64)
    assert nb * S["timing"]["block"] > c["kTimMaxBlocks"] * c["kTimNT"] * c["kTimG"]
    assert T.MAX_CALL_BLOCKS <= c["kTimScanPer"] * c["kTimNT"]
    assert T.MAX_CALL_BLOCKS * S["timing"]["block"] <= c["kTimMaxBlocks"] * c["kTimNT"] * c["kTimG"]

    c, _ = _consts("modem_frame.hip")
    ci, _ = _consts("modem_internal.h")
    decided = S["frame"]["nsym"] - S["frame"]["W"] - S["frame"]["L"] + 1
    tiles = (decided + ci["kFrameTile"] - 1) // ci["kFrameTile"]
    per_round = c["kFrScanPer"] * c["kFrNT"]
    assert tiles > per_round + 3 and decided % ci["kFrameTile"]                 # frame_scan_kernel, a partial last tile
    assert per_round * ci["kFrameTile"] == 1024 * 256                           # where the test plants its words
    assert S["gather"]["cap"] > c["kFrMaxBlocks"]                               # frame_gather_kernel

    c, text = _consts("modem_chan.hip")
    per_trip = c["kChanMaxBlocks"] * c["kChanNT"] * c["kChanG"]
    assert S["chan"]["n"] > per_trip and (S["chan"]["n"] - per_trip) % (c["kChanNT"] * c["kChanG"])
    cap = re.search(r"count_errors_kernel, dim3\(\(unsigned\)\(nblk < (\d+) \? nblk : (\d+)\)\)", text)
    assert cap and cap.group(1) == cap.group(2)
    lanes = int(cap.group(1)) * c["kCountNT"]
    work = lambda n, head: (n - head) // 16 + head + 16                       # launch_count_errors  # noqa: E731
    assert work(S["count_aligned"]["n"], 0) > lanes + 16
    assert work(S["count_bytewise"]["n"], S["count_bytewise"]["n"]) > lanes + 16
    assert work(S["count_common"]["n"], 16 - S["count_common"]["skew"]) > lanes + 16

    c, _ = _consts("modem_demap.hip")
    assert S["demap"]["nsym"] > c["kDemapMaxBlocks"] * c["kDemapNT"] and S["demap"]["nsym"] % c["kDemapNT"]
    c, _ = _consts("modem_noncoh.hip")
    assert S["diff"]["nsym"] > c["kDiffMaxBlocks"] * c["kDiffNT"] and S["diff"]["nsym"] % c["kDiffNT"]

    c, _ = _consts("modem_fec.hip")
    for name in ("encode_k3", "encode_k7"):
        steps = S[name]["nframes"] * (S[name]["nbits"] + S[name]["K"] - 1)
        assert steps > c["kEncMaxBlocks"] * c["kEncNT"]
