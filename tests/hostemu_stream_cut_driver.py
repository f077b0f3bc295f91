"""TEST INFRASTRUCTURE: the host side of the cut of a closed stream batch (csrc/tpt_frame_pools.h), driven through csrc/tpt_host*.cpp
compiled against tests/hostemu's stand-in for the HIP runtime (tests/test_stream_cut_host.py runs it with TPT_LIB=tests/_build/
libtpt_hostemu_stream_cut.so, which adds tests/hostemu_stream_cut.cpp's look at the launch queue and the cut words).  When a STREAM entry
with unserved frames is dropped, its slot's word must hold serial << 8 | frames served; a batch served in full writes nothing.  The
emulated kernels ignore the word (every frame is traced), which a cut permits: images and ray totals are held against the oracle.
Prints one line per scenario."""
import ctypes as C
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
W, H, SPP = 72, 40, 2  # 5.8 K samples: 8 frames per STREAM launch, 45 chunks per frame
FRAMES = 14
lib = None
_ORACLE = None


def oracle():
    global _ORACLE
    if _ORACLE is None:
        _ORACLE = oracle_frames(o, W, H, SPP, FRAMES, seed_mode=SEED_PER_PIXEL)
    return _ORACLE


def front():
    out = (C.c_int * 4)()
    return tuple(out) if lib.hostemuStreamFront(out) else None


def draw(tile, frames):
    for f in frames:
        tpt.UpdateTest(0.0, f, W, H, FLAG_PROGRESSIVE)
        tpt.draw_device(0.0, f, W, H, tile.ctypes.data, FLAG_PROGRESSIVE)


def start(served):
    """frames 0 and 1 plain, then one STREAM launch of frames 2..9 of which `served` are asked -> (tile, r0, its queue entry)"""
    tpt.set_samples_per_pixel(SPP)
    tpt.set_stream_batching(1)
    tpt.set_frame_overlap(16)
    tpt.set_host_lookahead(0)  # (the emulated device may finish a frame before the next call: the caller must not look synchronous)
    tpt.synchronize()
    tile = np.zeros((H, W, 4), np.float32)
    r0 = tpt.ray_counter_read()
    draw(tile, range(0, 3))
    first = front()
    assert first is not None and first[2:] == (1, 8), first  # (served on push: one frame of eight)
    slot, serial = first[0], first[1]
    assert serial != 0, "the launch has no pool per frame: the case no longer exercises the cut (grid %d)" % tpt.launch_info()["grid_blocks"]
    assert serial == lib.hostemuNewestCutSerial() and 1 <= serial < (1 << 24)
    assert lib.hostemuCutWord(slot) == 0, "a launch starts with its word at 0"
    draw(tile, range(3, 2 + served))
    if served < 8:
        assert front() == (slot, serial, served, 8), front()
        assert lib.hostemuCutWord(slot) == 0, "nothing is written while the entry is open"
    else:
        assert front() is None
    return tile, r0, slot, serial


def finish(tile, r0, first):
    """the stream goes on after the wait: frame `first` starts a launch of its own, with the next serial and its word at 0"""
    serial_before = lib.hostemuNewestCutSerial()
    draw(tile, [first])
    f = front()
    assert f is not None and f[1] == serial_before + 1 and f[2] == 1 and lib.hostemuCutWord(f[0]) == 0, (f, serial_before)
    draw(tile, range(first + 1, FRAMES))
    tpt.synchronize()
    total, want, per_frame = oracle()
    rays = tpt.ray_counter_read() - r0
    assert rays == total, (rays, total)
    assert tile.tobytes() == want.tobytes(), "tile differs from the oracle after a cut stream"
    tpt.set_host_lookahead(2)


def cut_by(wait, served):
    tile, r0, slot, serial = start(served)
    wait()
    assert front() is None
    word = lib.hostemuCutWord(slot)
    assert word == (serial << 8 | served), "slot %d holds %#x, expected serial %#x keep %d" % (slot, word, serial, served)
    finish(tile, r0, 2 + served)
    return "slot %d word %#x" % (slot, word)


def timer_end():
    tpt.timer_end()


def discard():
    tpt.set_host_lookahead(0)  # (drops what was traced ahead: LaunchQueue::discard)


def fully_served():
    tile, r0, slot, serial = start(8)
    tpt.synchronize()
    assert lib.hostemuCutWord(slot) == 0, "a batch served in full was cut"
    tpt.timer_begin()
    tpt.timer_end()
    assert lib.hostemuCutWord(slot) == 0
    finish(tile, r0, 10)


SCENARIOS = [("tptSynchronize cuts, keep %d" % k, (lambda k=k: cut_by(tpt.synchronize, k))) for k in (1, 3, 7)] + [
    ("tptRayCounterRead cuts", lambda: cut_by(tpt.ray_counter_read, 2)),
    ("tptTimerEnd cuts", lambda: (tpt.timer_begin(), cut_by(timer_end, 5))[1]),
    ("discard cuts", lambda: cut_by(discard, 4)),
    ("a batch served in full writes nothing", fully_served),
]

if __name__ == "__main__":
    tpt.InitializeTest()
    lib = C.CDLL(os.environ["TPT_LIB"])
    lib.hostemuCutWord.restype = C.c_uint
    lib.hostemuNewestCutSerial.restype = C.c_uint
    failed = 0
    for name, fn in SCENARIOS:
        try:
            extra = fn()
            print("OK   %s%s" % (name, "" if extra is None else "  %s" % (extra,)), flush=True)
        except Exception as e:  # noqa: BLE001
            failed += 1
            tpt.synchronize()  # (queued work still writes the scenario's tile: drain it while the traceback keeps the tile alive)
            print("FAIL %s: %s: %s" % (name, type(e).__name__, e), flush=True)
    tpt.ShutdownTest()
    sys.exit(1 if failed else 0)
