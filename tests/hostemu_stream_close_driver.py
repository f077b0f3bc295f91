"""TEST INFRASTRUCTURE: a caller that waits in the middle of a stream (tptSynchronize, tptRayCounterRead) while a STREAM batch is open,
driven through csrc/tpt_host.cpp compiled against tests/hostemu's stand-in for the HIP runtime (tests/test_stream_close.py runs it with
TPT_LIB=tests/_build/libtpt_hostemu.so).  The call after the wait must be traced anew, not served from a plane traced before it; images
and ray totals are held against the oracle.  Prints one line per scenario."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from common import oracle_frames  # noqa: E402
from oracle_lib import FLAG_PROGRESSIVE, SEED_PER_PIXEL, Oracle  # noqa: E402

assert "hostemu" in os.environ.get("TPT_LIB", ""), "this driver is for the host-emulation build only"
from toypathtracer_amd import api as tpt  # noqa: E402

o = Oracle.get()
W, H, SPP = 32, 24, 2  # 1.5 K samples: 8 frames per STREAM launch


def draw(tile, frames):
    for f in frames:
        tpt.UpdateTest(0.0, f, W, H, FLAG_PROGRESSIVE)
        tpt.draw_device(0.0, f, W, H, tile.ctypes.data, FLAG_PROGRESSIVE)


def wait_mid_stream(wait):
    """frames 0-4 (0 and 1 plain, 2-9 one STREAM launch), the wait, then frames 5-12: frame 5 starts a launch of its own (5-12), 6-12
    are served from it"""
    tpt.set_samples_per_pixel(SPP)
    tpt.set_stream_batching(1)
    tpt.set_frame_overlap(16)
    tpt.set_host_lookahead(0)  # (the emulated device may finish a frame before the next call: the caller must not look synchronous)
    tpt.synchronize()
    tile = np.zeros((H, W, 4), np.float32)
    r0 = tpt.ray_counter_read()
    tpt.kernel_timing_begin(16)
    draw(tile, range(0, 5))
    _, before = tpt.kernel_timing_end()
    assert before == 3, before  # (two plain launches and the batch)
    mid = wait()
    tpt.kernel_timing_begin(16)
    draw(tile, [5])
    _, first = tpt.kernel_timing_end()
    assert first == 1, "frame 5 was served from a launch traced before the wait (%d launches)" % first
    tpt.kernel_timing_begin(16)
    draw(tile, range(6, 13))
    _, rest = tpt.kernel_timing_end()
    assert rest == 0, rest
    tpt.synchronize()
    rays = tpt.ray_counter_read() - r0
    total, want, per_frame = oracle_frames(o, W, H, SPP, 13, seed_mode=SEED_PER_PIXEL)
    if mid is not None:
        assert mid - r0 == sum(per_frame[:5]), (mid - r0, sum(per_frame[:5]))  # exact at the wait: frames 5-9 of the dropped batch never counted
    assert rays == total, (rays, total)
    if tile.tobytes() != want.tobytes():
        raise AssertionError("tile differs from the oracle after a wait in the stream")
    tpt.set_host_lookahead(2)


def wait_keeps_lookahead():
    """a synchronous caller's frames traced ahead (AHEAD) survive its synchronise: from the third frame on every call is a hit"""
    tpt.set_samples_per_pixel(SPP)
    tpt.set_host_lookahead(2)
    tpt.synchronize()
    tile = np.zeros((H, W, 4), np.float32)
    hits0 = tpt.lookahead_hits()
    for f in range(8):
        draw(tile, [f])
        tpt.synchronize()
    hits = tpt.lookahead_hits() - hits0
    _, want, _ = oracle_frames(o, W, H, SPP, 8, seed_mode=SEED_PER_PIXEL)
    assert tile.tobytes() == want.tobytes()
    assert hits >= 4, hits
    return hits


SCENARIOS = [
    ("synchronise in an open stream batch", lambda: wait_mid_stream(lambda: (tpt.synchronize(), None)[1])),
    ("ray counter read in an open stream batch", lambda: wait_mid_stream(tpt.ray_counter_read)),
    ("look-ahead kept across synchronise", wait_keeps_lookahead),
]

if __name__ == "__main__":
    tpt.InitializeTest()
    failed = 0
    for name, fn in SCENARIOS:
        try:
            extra = fn()
            print("OK   %s%s" % (name, "" if extra is None else "  %s" % (extra,)), flush=True)
        except Exception as e:  # noqa: BLE001
            failed += 1
            print("FAIL %s: %s: %s" % (name, type(e).__name__, e), flush=True)
    tpt.ShutdownTest()
    sys.exit(1 if failed else 0)
