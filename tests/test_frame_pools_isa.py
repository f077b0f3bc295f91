"""The gfx950 code of tptFramePoolsKernel (the batched path-queue kernel with a pool of chunks per frame) inside the shipped library: the
contract tests/test_isa_contract.py states for tptTraceQueueKernel<., true>, for its twin, and the selection of the variant on the host."""
import os
import subprocess

import pytest

from isa_lib import HAVE_TOOLS, code_object, count  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import POOLS, QUEUE, family
from oracle_lib import ROOT

needs_tools = pytest.mark.skipif(not HAVE_TOOLS, reason="ROCm LLVM tools not installed")


@needs_tools
@pytest.mark.parametrize("lds", [1, 0], ids=["lds-scene", "grouped"])
def test_frame_pools_kernels_keep_their_twins_contract(code_object, lds):  # noqa: F811
    bodies, meta = code_object
    name, twin = POOLS % lds, QUEUE % (lds, 1)
    assert name in meta and name in bodies, "the frame-pools kernel is missing from the shipped code object"
    body, m, t = bodies[name], meta[name], meta[twin]
    assert count(body, r"flat_") == 0, "a FLAT instruction: an LDS pointer lost its address space"
    assert count(body, r"buffer_(load|store|atomic)") == 0
    assert count(body, r"ds_(read|load)") >= 30 and count(body, r"ds_(write|store)") >= 15
    assert m["group_segment_fixed_size"] == t["group_segment_fixed_size"]
    assert m["agpr_count"] == 0 and m["max_flat_workgroup_size"] == 512 and m["wavefront_size"] == 64
    assert count(body, r"v_mfma") == count(body, r"v_mfma_f32_32x32x16_f16") == count(bodies[twin], r"v_mfma")
    if lds:
        # four waves per SIMD with room for the blend's waves beside them; what is parked in scratch are binary64 constants of
        # pow5 / sin-cos hoisted to the kernel's entry: a store each there, a load each in the class code, none in the intersection
        assert m["vgpr_count"] <= 120, m
        assert m["vgpr_spill_count"] <= 4 and m["private_segment_fixed_size"] <= 20, m
        assert count(body, r"scratch_store") == count(body, r"scratch_load") <= 2
    else:
        assert m["vgpr_count"] <= 128, m
    # a workgroup counts its rays per lane for its one frame: fewer LDS atomics than the twin, which counts per frame
    assert count(body, r"ds_add") < count(bodies[twin], r"ds_add")


@needs_tools
def test_the_new_kernels_are_counted_by_no_other_test(code_object):  # noqa: F811
    """(no test counts kernels by the words in their names any more: tests/test_isa_contract.py holds the library to the manifest)"""
    _, meta = code_object
    assert sorted(n for n in meta if "FramePools" in n) == sorted(family(POOLS))


VARIANT_PROGRAM = r'''
#include <cstdio>
#include <initializer_list>
#include "tpt_queue_layout.h"
using namespace tpt;
int main()
{
    static CameraPOD cams[32];
    static f4 centres[64], sums[3];
    KernelArgs a{};
    a.scene.nPairs = 23; a.scene.nSpheres = 46; a.scene.nLights = 2; a.scene.mxR1 = 0; // (the built-in scene)
    a.fc.seedMode = SEED_PER_PIXEL;
    a.batchFrames = 8;
    printf("shared %d\n", (int)(tptQueueVariant(a) == QV_BATCH));
    const size_t shared = tptQueueLdsBytes(a, true);
    a.framePools = 8;
    printf("pools %d\n", (int)(tptQueueVariant(a) == QV_FRAME_POOLS));
    printf("lds %d\n", (int)(tptQueueLdsBytes(a, true) == shared));
    for (int n : {2, 5}) { a.batchFrames = a.framePools = n; printf("frames-%d %d\n", n, (int)(tptQueueVariant(a) == QV_FRAME_POOLS)); }
    a.batchFrames = a.framePools = 1; printf("invalid one %d\n", (int)(tptQueueVariant(a) == QV_INVALID));
    a.batchFrames = a.framePools = 9; printf("invalid nine %d\n", (int)(tptQueueVariant(a) == QV_INVALID));
    a.batchFrames = 8; a.framePools = 4; printf("invalid fewer %d\n", (int)(tptQueueVariant(a) == QV_INVALID));
    a.framePools = 8;
    a.helperBase = 512; printf("invalid helper %d\n", (int)(tptQueueVariant(a) == QV_INVALID)); a.helperBase = 0;
    a.viewCams = cams; printf("invalid views %d\n", (int)(tptQueueVariant(a) == QV_INVALID)); a.viewCams = nullptr;
    a.moveCentres = centres; printf("invalid animation %d\n", (int)(tptQueueVariant(a) == QV_INVALID)); a.moveCentres = nullptr;
    a.aovSums = sums; printf("invalid planes %d\n", (int)(tptQueueVariant(a) == QV_INVALID)); a.aovSums = nullptr;
    a.fc.seedMode = SEED_ROW_SERIAL; printf("invalid row-serial %d\n", (int)(tptQueueVariant(a) == QV_INVALID)); a.fc.seedMode = SEED_PER_PIXEL;
    printf("valid %d\n", (int)(QV_FRAME_POOLS < QV_INVALID));
    return 0;
}
'''


def test_variant_on_the_host(tmp_path):
    src, exe = str(tmp_path / "variant.cpp"), str(tmp_path / "variant")
    open(src, "w").write(VARIANT_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-include", "hip/hip_runtime.h",
                           "-I", os.path.join(ROOT, "tests", "hostemu"), "-I", os.path.join(ROOT, "toypathtracer_amd", "csrc"), src, "-o", exe])
    out = dict(ln.rsplit(" ", 1) for ln in subprocess.check_output([exe]).decode().splitlines())
    assert len(out) == 14 and all(v == "1" for v in out.values()), out
