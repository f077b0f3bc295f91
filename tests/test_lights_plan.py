"""What the host's plan (chooseKernel, csrc/tpt_host_pipeline.cpp) does with the LIGHT LIST, without a GPU: the host code, unmodified,
on the emulation build (tests/test_host_logic.py: build) in child processes (tests/lights_plan_child.py), every image and ray count
held against the oracle.  The scenes are tests/lights_lib.py's; tests/test_gpu_lights.py runs the same ones through the real kernels.

  - the 15 / 16 seam of the built-in scene: the 16th light costs the scene its place in LDS, not the CU its second workgroup;
  - 0, 1, 16 and 46 lights, and every kind of light (metal, glass, the ground, enclosing, tiny, huge, ...);
  - the 4096-sphere scene at 2864 lights (the path-queue kernel's LDS is exactly a CU's: one workgroup per CU, never 0), 2865 and 3072
    (past what that kernel holds: the lane-refill kernel takes the frame), 3073 (refused by the stated cap, include/tpt_hip.h);
  - the entry points behind the same limit: a stream of frames and tptDrawDeviceAnimation go frame by frame, tptDrawDeviceBatch says
    how many lights it takes.

TEST INFRASTRUCTURE: nothing here is reachable from the product."""
import json
import os
import re
import subprocess
import sys

import pytest

import lights_lib
from oracle_lib import ROOT
from test_host_logic import build

HERE = os.path.dirname(os.path.abspath(__file__))
CU_LDS = 160 * 1024  # gfx950: LDS of a CU, and the most one workgroup may take


def header_light_cap():
    text = open(os.path.join(ROOT, "include", "tpt_hip.h")).read()
    caps = re.findall(r"^#define TPT_MAX_LIGHTS (\d+)$", text, re.M)
    assert len(caps) == 1, "include/tpt_hip.h states the light cap once"
    return int(caps[0])


@pytest.fixture(scope="module")
def seen():
    """every section at once, one process each (the 4096-sphere sections are about a minute of emulation and oracle)"""
    lib = build("libtpt_hostemu.so", [])
    env = dict(os.environ, TPT_LIB=lib, HOSTEMU_POLICY="eager")
    env.pop("TPT_LIB_DIR", None)
    jobs = {k: subprocess.Popen([sys.executable, os.path.join(HERE, "lights_plan_child.py"), k], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            for k in ("counts", "kinds", "plan", "fallbacks")}
    out = {}
    for k, p in jobs.items():
        text = p.communicate(timeout=900)[0].decode()
        assert p.returncode == 0, "%s:\n%s" % (k, text[-3000:])
        out[k] = json.loads(text.strip().splitlines()[-1])
    return out


def equals_oracle(r):
    assert r["refused"] is None, r
    assert r["finite"], "the oracle's own image is not finite: the scene is no fair test (tests/lights_lib.py)"
    assert r["rays_equal"] and r["image_equal"], r


def test_the_header_states_the_cap():
    assert header_light_cap() == 3072


@pytest.mark.parametrize("k", [0, 1, 15, 16, 46])
def test_light_counts_equal_the_oracle(seen, k):
    r = seen["counts"]["%d" % k]
    equals_oracle(r)
    assert r["lit"] or k == 0


def test_the_16th_light_costs_the_lds_scene_not_the_second_workgroup(seen):
    """two workgroups per CU are worth more than the scene in LDS"""
    a, b = seen["counts"]["15"], seen["counts"]["16"]
    assert a["blocks_per_cu"] == 2 and b["blocks_per_cu"] == 2
    assert b["lds_bytes"] < a["lds_bytes"], "16 lights still stage the scene in LDS: the seam moved (tests/lights_lib.py LIGHT_COUNTS straddles it)"
    # the scene forced into LDS beside the 16th light is what the plan avoids: 32 bytes more, and the second workgroup is gone
    forced = seen["counts"]["16 lds_scene 1"]
    equals_oracle(forced)
    assert forced["lds_bytes"] == a["lds_bytes"] + 32 and forced["blocks_per_cu"] == 1, forced
    # the lane-refill kernel has no such seam: one light more is 32 bytes more
    equals_oracle(seen["counts"]["15 lane-refill"])
    equals_oracle(seen["counts"]["16 lane-refill"])
    assert seen["counts"]["16 lane-refill"]["lds_bytes"] - seen["counts"]["15 lane-refill"]["lds_bytes"] == 32


@pytest.mark.parametrize("kernel", ["", " lane-refill"], ids=["path_queues", "lane_refill"])
@pytest.mark.parametrize("kind", lights_lib.LIGHT_KINDS)
def test_light_kinds_equal_the_oracle(seen, kind, kernel):
    r = seen["kinds"][kind + kernel]
    equals_oracle(r)
    assert r["lit"]
    assert r["div_safe"] == (kind not in ("tiny", "huge")), "tiny and huge are the scenes that clear SCENE_LIGHT_R2_DIV_SAFE"


def test_2864_lights_fill_a_cu_and_still_count_as_one_workgroup(seen):
    r = seen["plan"]["2864"]
    equals_oracle(r)
    assert r["lds_bytes"] == CU_LDS, "2864 lights no longer fill the path-queue kernel's LDS exactly: pick the count that does"
    assert r["blocks_per_cu"] == 1
    assert r["grid_blocks"] >= 1


@pytest.mark.parametrize("k", [2865, 3072])
def test_more_lights_than_the_path_queue_kernel_holds_take_the_lane_refill_kernel(seen, k):
    r = seen["plan"]["%d" % k]
    equals_oracle(r)
    assert r["blocks_per_cu"] >= 1 and r["lds_bytes"] <= CU_LDS
    assert r["lds_bytes"] - 32 * k < 32 * 1024, "not the lane-refill kernel's LDS (the light table and a few levels of bounce stack)"
    assert seen["plan"]["2865 lds_scene 0"]["refused"] is None


def test_3073_lights_are_refused_by_the_stated_cap(seen):
    cap = header_light_cap()
    for key in ("3073", "3073 lds_scene 0"):
        msg = seen["plan"][key]["refused"]
        assert msg and "too many emissive spheres" in msg and "%d at most" % cap in msg, msg
        assert "tptSetKernelVariant" not in msg, "advice that cannot help"
    assert seen["plan"]["3073"]["untouched"]
    after = seen["plan"]["after"]  # the next draw, of the built-in scene
    equals_oracle(after)
    assert after["blocks_per_cu"] == 2


def test_entry_points_behind_the_same_limit(seen):
    f = seen["fallbacks"]
    for key in ("stream", "animation"):  # frame by frame on the lane-refill kernel
        assert f[key]["image_equal"] and f[key]["rays_equal"], (key, f[key])
        assert f[key]["blocks_per_cu"] >= 1 and f[key]["lds_bytes"] - 32 * 3072 < 32 * 1024
    msg = f["batch"]["refused"]  # no such way out: the count and the call's own limit
    assert msg and "3072 emissive spheres" in msg and "at most 2864" in msg and "tptSetKernelVariant" not in msg, msg
    assert f["batch"]["untouched"]
