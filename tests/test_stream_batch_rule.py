"""The frames per STREAM launch (csrc/tpt_stream_batch.h), on the CPU: the header the host runtime includes, compiled for the host
(tests/stream_batch_shim.cpp -> tests/_build/).  The depth comes from a number of hardware queues through the same clamp the runtime
applies to its probe (1, 2 and 4 queues: two frames in flight; 16: the full pipeline)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "toypathtracer_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "stream_batch_shim.cpp")
HDR = os.path.join(INC, "tpt_stream_batch.h")


@pytest.fixture(scope="module")
def rule():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libstream_batch_shim.so")
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in (SRC, HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", INC, SRC, "-o", so])
    lib = C.CDLL(so)
    lib.sb_frames.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_longlong]
    return lib


def frames(rule, w, h, spp, queues, run=8):
    """frames per launch for a streaming caller of w x h x spp frames with `queues` hardware queues, `run` batches into the stream"""
    depth = min(rule.sb_overlap_cap(queues), rule.sb_max_overlap())
    return rule.sb_frames(w * h * spp, depth, run, w * h * 16)


def old_rule(samples):
    """the rule before the pipeline depth entered it (frame size only)"""
    return 1 if samples >= 2400000 else 2 if samples >= 1200000 else 4 if samples >= 600000 else 8


def test_queue_clamp_is_unchanged(rule):
    """the depth the runtime derives from its queue probe (tests/test_gpu_api.py pins overlap_effective on the GPU)"""
    assert [rule.sb_overlap_cap(q) for q in (1, 2, 3, 4, 7, 8, 12, 15, 16, 20)] == [2, 2, 2, 2, 2, 5, 9, 12, 16, 16]


@pytest.mark.parametrize("queues", [1, 2, 4, 16])
def test_small_frames_keep_their_batch_sizes(rule, queues):
    """frames under 2.4 M samples get 2 / 4 / 8 frames per launch at every depth and from the first batch of a stream on"""
    for w, h, spp in [(32, 24, 2), (256, 144, 4), (640, 360, 1), (640, 360, 4), (960, 540, 1), (1280, 720, 1), (1280, 720, 2),
                      (1000, 600, 2), (1920, 1080, 1), (700, 500, 5)]:
        for run in (0, 1, 5):
            assert frames(rule, w, h, spp, queues, run) == old_rule(w * h * spp), (w, h, spp, queues, run)


def test_deep_pipeline_keeps_one_frame_per_launch_at_1280x720(rule):
    """16 queues: one frame per launch for every frame of 2.4 M samples and more, as before (the 20-queue headline)"""
    assert frames(rule, 1280, 720, 4, 16) == 1
    for w, h, spp in [(1280, 720, 4), (1920, 1080, 8), (3840, 2160, 16), (2400, 1000, 1)]:
        for run in (0, 3, 9):
            assert frames(rule, w, h, spp, 16, run) == 1, (w, h, spp, run)


@pytest.mark.parametrize("queues", [1, 2, 4])
def test_shallow_pipeline_batches_1280x720(rule, queues):
    """two frames in flight: 1280x720x4 gets several frames per launch, 2 / 4 / 8 as the stream goes on, never more than the cap"""
    assert [frames(rule, 1280, 720, 4, queues, run) for run in range(5)] == [2, 4, 8, 8, 8]
    assert frames(rule, 3840, 2160, 16, queues) == 1  # (132 M samples: one frame is as long as sixteen launches of the deep pipeline)


def test_batch_follows_the_depth(rule):
    """the launches in flight carry about what sixteen launches of 2.4 M samples did: fewer frames per launch as the pipeline deepens"""
    s = 1280 * 720 * 4
    got = [rule.sb_frames(s, d, 8, 1280 * 720 * 16) for d in (1, 2, 3, 4, 5, 8, 9, 12, 16)]
    assert got == [1, 8, 4, 4, 4, 2, 2, 1, 1], got
    for d in range(2, 17):
        k = rule.sb_frames(s, d, 8, 1280 * 720 * 16)
        assert 1 <= k <= rule.sb_batch_max()
        assert k == 1 or (k // 2) * d * s < 16 * 2400000  # (the smallest power of two that reaches the deep pipeline's work)


def test_colour_memory_caps_the_batch(rule):
    """the colour planes of the launches in flight stay under 1 GiB: a frame of 256 MiB colour gets fewer frames per launch"""
    assert rule.sb_frames(2400000, 2, 8, 64 << 20) == 8
    assert rule.sb_frames(2400000, 2, 8, 128 << 20) == 4
    assert rule.sb_frames(2400000, 2, 8, 600 << 20) == 1
