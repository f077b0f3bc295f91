"""The seventh ring of the frame-pools kernel for scenes staged in LDS (csrc/tpt_queue_layout.h, Q_LAST) in the shipped gfx950 code, and
what it costs in LDS: nothing.  The grouped instantiation keeps six rings and its 608 paths (it measured slower with the split).

Every wave starts an iteration by reading "tail - head" of ring c in lane c and broadcasting the word with one v_readlane_b32 per ring,
lane indices 0, 1, 2, ... as immediates, all from one VGPR and next to each other (seen in the build: lane 0, five other instructions,
then lanes 1 .. 5 -- 1 .. 6 in tptFramePoolsKernel<true> -- back to back).  The number of those reads is the instantiation's ring count."""
import os
import re
import subprocess

import pytest

from isa_lib import HAVE_TOOLS, code_object  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import POOLS, QUEUE
from oracle_lib import ROOT

needs_tools = pytest.mark.skipif(not HAVE_TOOLS, reason="ROCm LLVM tools not installed")
WINDOW = 16  # instructions from the read of lane 0 within which the other rings' reads stand


def rings_in_the_pick(body):
    """the longest run 0, 1, 2, ... of immediate lane indices read from one VGPR by v_readlane_b32 within WINDOW instructions of its
    lane-0 read (a register that holds spilled SGPRs is read a lane or two at a time, far apart)"""
    best = 0
    for i, ins in enumerate(body):
        if ins and ins[0] == "v_readlane_b32" and ins[-1] == "0":
            src = ins[2]
            lanes = {int(j[-1]) for j in body[i:i + WINDOW] if j and j[0] == "v_readlane_b32" and j[2] == src and re.fullmatch(r"\d+", j[-1])}
            run = 0
            while run in lanes:
                run += 1
            best = max(best, run)
    return best


@needs_tools
def test_the_lds_scene_pools_kernel_picks_among_seven_rings_the_others_among_six(code_object):  # noqa: F811
    bodies, _ = code_object
    counts = {name: rings_in_the_pick(bodies[name]) for name in [POOLS % 1, POOLS % 0, QUEUE % (1, 0), QUEUE % (1, 1)]}
    print(counts)
    assert counts[POOLS % 1] == 7 and counts[POOLS % 0] == 6, counts
    assert counts[QUEUE % (1, 0)] == 6 and counts[QUEUE % (1, 1)] == 6, counts


LDS_PROGRAM = r'''
#include <cstdio>
#include <initializer_list>
#include "tpt_queue_layout.h"
using namespace tpt;
int main()
{
    KernelArgs a{};
    a.fc.seedMode = SEED_PER_PIXEL;
    a.scene.nPairs = 23; a.scene.nSpheres = 46; a.scene.nLights = 2; a.scene.mxR1 = 0; // (the built-in scene)
    for (int frames : {2, 8}) {
        a.batchFrames = frames; a.framePools = 0;
        const bool shared = tptQueueVariant(a) == QV_BATCH;
        const size_t lds = tptQueueLdsBytes(a, true), grouped = tptQueueLdsBytes(a, false);
        a.framePools = frames;
        printf("pools-%d %d\n", frames, (int)(shared && tptQueueVariant(a) == QV_FRAME_POOLS));
        printf("lds-scene-%d %d\n", frames, (int)(tptQueueLdsBytes(a, true) == lds));
        printf("grouped-%d %d\n", frames, (int)(tptQueueLdsBytes(a, false) == grouped));
    }
    // the ring is paid for by path records of the LDS-scene instantiation: as many bytes
    printf("ring-bytes %d\n", (int)(TPT_Q_LAST_PATHS * TPT_Q_NF4 * 16 == TPT_Q_P * 2 && (int)Q_COUNT_POOLS == (int)Q_COUNT + 1 && (int)Q_LAST == (int)Q_COUNT));
    printf("paths %d\n", (int)(TPT_Q_PATHS - TPT_Q_LAST_PATHS == 920 && TPT_Q_LAST_PATHS == 32));
    printf("heads %d\n", (int)(Q_COUNT_POOLS <= (int)(sizeof(QueueCtl::head) / 4) && Q_COUNT_POOLS <= (int)(sizeof(QueueCtl::tail) / 4)));
    return 0;
}
'''


def test_a_pools_launch_takes_its_twins_lds(tmp_path):
    src, exe = str(tmp_path / "lds.cpp"), str(tmp_path / "lds")
    open(src, "w").write(LDS_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-include", "hip/hip_runtime.h",
                           "-I", os.path.join(ROOT, "tests", "hostemu"), "-I", os.path.join(ROOT, "toypathtracer_amd", "csrc"), src, "-o", exe])
    out = dict(ln.rsplit(" ", 1) for ln in subprocess.check_output([exe]).decode().splitlines())
    assert len(out) == 9 and all(v == "1" for v in out.values()), out
