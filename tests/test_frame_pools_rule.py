"""A pool of chunks per frame of a batched launch (csrc/tpt_frame_pools.h), on the CPU: the header the kernel and the host runtime
include, compiled for the host (tests/frame_pools_shim.cpp -> tests/_build/)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "toypathtracer_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "frame_pools_shim.cpp")
HDR = os.path.join(INC, "tpt_frame_pools.h")


@pytest.fixture(scope="module")
def rule():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libframe_pools_shim.so")
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in (SRC, HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", INC, SRC, "-o", so])
    return C.CDLL(so)


def test_counters_fit_the_launch_counter_block(rule):
    """work[] is 16 words per slot, [0..3] in use: the pools of the largest stream batch (8 frames) sit in work[4..11]"""
    assert rule.fp_base() == 4 and rule.fp_max() == 8
    assert rule.fp_base() + rule.fp_max() <= 16


@pytest.mark.parametrize("batch", range(2, 9))
def test_every_frame_gets_its_share_of_the_grid(rule, batch):
    for blocks in range(16, 1025):
        frames = [rule.fp_frame_of_block(b, batch, blocks) for b in range(blocks)]
        assert frames[0] == 0 and frames[-1] == batch - 1, (batch, blocks)
        assert all(0 <= y - x <= 1 for x, y in zip(frames, frames[1:])), (batch, blocks)  # monotonic, no frame skipped
        counts = [frames.count(f) for f in range(batch)]
        assert min(counts) >= 1 and max(counts) - min(counts) <= 1, (batch, blocks, counts)
        assert min(counts) >= 2  # (the rule below asks for 2 x batch workgroups: 16 is enough for every batch)


def test_shared_pool_exactly_outside_the_conditions(rule):
    for batch in range(0, 40):
        for blocks in list(range(0, 70)) + [127, 128, 512, 1024]:
            for plain in (0, 1):
                for helpable in (0, 1):
                    want = batch if (plain and not helpable and 2 <= batch <= 8 and blocks >= 2 * batch) else 0
                    assert rule.fp_pools(batch, blocks, plain, helpable) == want, (batch, blocks, plain, helpable)


def test_smallest_grids_of_the_rule(rule):
    """2 x batch workgroups, the fewest the rule takes: two per frame"""
    for batch in range(2, 9):
        blocks = 2 * batch
        assert rule.fp_pools(batch, blocks, 1, 0) == batch and rule.fp_pools(batch, blocks - 1, 1, 0) == 0
        assert [rule.fp_frame_of_block(b, batch, blocks) for b in range(blocks)] == [b // 2 for b in range(blocks)]
