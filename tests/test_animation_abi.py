"""tptDrawDeviceAnimation without a GPU: the declaration, the binding and the export of the entry point; HitSpheres of the animation
kernel over a batch -- one staged scene's filter, each frame's moving centres -- restated on the host (tests/animation_filter.cpp) and
held against each frame's reference test on near-tangent rays; the gfx950
code of the animation kernels in the shipped library (the contract of the views kernels, tests/test_views_abi.py); and the refusals,
driven through the host runtime compiled against tests/hostemu (a refused call returns before anything is enqueued)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from isa_lib import code_object, count, exported_symbols, header_params, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import ANIM, QUEUE
from oracle_lib import ROOT

INC = os.path.join(ROOT, "toypathtracer_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "animation_filter.cpp")


def test_header_declares_the_entry_point():
    params = header_params("tptDrawDeviceAnimation")
    assert params == ["int firstFrame", "int nFrames", "const float* times", "int screenWidth", "int screenHeight", "float* deviceTile",
                      "float* deviceFrameImages", "int64_t* deviceFrameRays", "unsigned testFlags"], params


def test_binding_and_export():
    from toypathtracer_amd import api
    assert "tptDrawDeviceAnimation" in api.C_ABI_SYMBOLS
    assert callable(api.draw_device_animation)
    lib = api.load_library()
    assert hasattr(lib, "tptDrawDeviceAnimation")
    assert re.search(r"\bT tptDrawDeviceAnimation\b", exported_symbols(api.library_path()))


def test_times_shape_is_checked_before_the_library():
    from toypathtracer_amd import api
    with pytest.raises(ValueError):
        api.draw_device_animation([[0.0, 1.0]], 0, 8, 8, 0, 3)


# ---------------------------------------------------------------- phase 1 + phase 2 of the animation kernel, restated on the host
@pytest.fixture(scope="module")
def shim():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libanimation_filter.so")
    deps = [SHIM] + [os.path.join(INC, f) for f in ("tpt_animation.h", "tpt_scene.h", "tpt_trace.h", "tpt_math.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas",
                               "-I", INC, SHIM, "-o", so])
    lib = C.CDLL(so)
    lib.an_filter_check.argtypes = [C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_ulonglong, C.c_void_p]
    lib.an_y1.argtypes = lib.an_z8.argtypes = [C.c_float]
    lib.an_y1.restype = lib.an_z8.restype = C.c_float
    return lib


@pytest.mark.parametrize("r1,r8,span", [(0.05, 0.02, 6.3), (0.01, 0.003, 1.0), (0.3, 0.3, 0.5), (0.05, 0.02, 1e4)],
                         ids=["rho-40-one-period", "rho-200", "default-radii", "many-periods"])
def test_filter_keeps_every_frames_hits_of_the_moving_spheres(shim, r1, r8, span):
    """One staged scene (the batch's last frame) serves 32 frames: on near-tangent rays of sphere 1 or 8 in each frame -- spheres that
    move up to hundreds of radii over the batch -- the matrix-core and the packed VALU paths give the reference's (id, t) bit for bit.
    The staged filter data alone would have dropped many of those hits: the forced candidates are what keeps them."""
    times = np.float32(np.linspace(-span / 2, span / 2, 32))
    out = np.zeros(5, np.int64)
    assert shim.an_filter_check(r1, r8, times.ctypes.data, len(times), 4000, 12345, out.ctypes.data) == 0
    rays, bad_matrix, bad_valu, dropped_without, hits = out.tolist()
    assert rays == 32 * 4000 and hits > rays // 4, out
    assert bad_matrix == 0 and bad_valu == 0, out
    if r1 < 0.1:
        assert dropped_without > hits // 4, out  # (the test has teeth: without forcing, the staged bounds miss these)


def test_centres_are_what_update_test_computes(shim):
    """the rule the runtime's tptUpdate uses too (Test.cpp:304-308): cosf(t) + 1, sinf(t) * 0.3 in binary32"""
    for t in (0.0, 0.5, 1.0, 3.14159, -7.25, 1e6):
        t32 = np.float32(t)
        assert abs(shim.an_y1(float(t32)) - (math.cos(float(t32)) + 1.0)) < 1e-6
        assert abs(shim.an_z8(float(t32)) - math.sin(float(t32)) * 0.3) < 1e-6


# ---------------------------------------------------------------- the shipped gfx950 code
@pytest.mark.parametrize("lds", [1, 0], ids=["lds-scene", "flat-global"])
def test_animation_kernels_keep_the_queue_kernel_contract(code_object, lds):  # noqa: F811
    bodies, meta = code_object
    name = ANIM % lds
    assert name in meta and name in bodies, "the animation kernel is missing from the shipped code object"
    body, m = bodies[name], meta[name]
    assert count(body, r"flat_") == 0, "a FLAT instruction: an LDS pointer lost its address space"
    assert count(body, r"ds_(read|load)") >= 30 and count(body, r"ds_(write|store)") >= 15
    assert m["agpr_count"] == 0
    assert m["vgpr_count"] <= 128, m
    assert m["max_flat_workgroup_size"] == 512 and m["wavefront_size"] == 64
    # the same matrix-core filter as its single-frame twin (8 MFMA for the <= 64-sphere table), none without the scene in LDS
    twin = bodies[QUEUE % (lds, 0)]
    assert count(body, r"v_mfma") == count(twin, r"v_mfma") == (8 if lds else 0)
    if lds:
        assert m["vgpr_count"] <= 120, m  # (as the single-frame kernel: the resolve kernel's waves start beside it)
        assert m["vgpr_spill_count"] <= meta[QUEUE % (1, 1)]["vgpr_spill_count"], m


def test_animation_kernel_takes_the_lds_of_its_single_frame_twin():
    """the centres table replaces path records byte for byte: tptQueueLdsBytes is unchanged by it, so the default scene keeps two
    workgroups per CU and the matrix-core filter (checked by the static_asserts of tpt_queue_layout.h, restated here from its constants)"""
    src = open(os.path.join(INC, "tpt_queue_layout.h")).read()
    assert "#define TPT_Q_ANIM_TABLE_BYTES (TPT_Q_VIEWS_MAX * 2 * 16)" in src
    assert "#define TPT_Q_ANIM_PATHS ((TPT_Q_ANIM_TABLE_BYTES + TPT_Q_NF4 * 16 - 1) / (TPT_Q_NF4 * 16))" in src
    assert re.search(r"#define TPT_Q_VIEWS_MAX 32\b", src) and re.search(r"#define TPT_Q_NF4 4\b", src)
    table, paths = 32 * 2 * 16, (32 * 2 * 16 + 4 * 16 - 1) // (4 * 16)
    assert table == 4 * 16 * paths == 1024 and paths == 16
    assert "if (moving) bytes += (size_t)TPT_Q_ANIM_TABLE_BYTES - (size_t)TPT_Q_NF4 * TPT_Q_ANIM_PATHS * 16;" in src
    assert 'static_assert(TPT_Q_ANIM_TABLE_BYTES == TPT_Q_NF4 * TPT_Q_ANIM_PATHS * 16' in src


# ---------------------------------------------------------------- refusals, through the host runtime
REFUSALS = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
tpt.InitializeTest()
w, h = 16, 8
tile = np.full((h, w, 4), 7.25, np.float32)
images = np.full((3, h, w, 4), -1.5, np.float32)
rays = np.full(3, -5, np.int64)
times = np.float32([0.0, 0.25, 0.5])
def refused(what, ww=w, hh=h, n=3, t=True, tl=True):
    rc = lib.tptDrawDeviceAnimation(0, n, times.ctypes.data if t else None, ww, hh, tile.ctypes.data if tl else None,
                                    images.ctypes.data, rays.ctypes.data, 3)
    msg = lib.tptGetLastError().decode()
    assert rc != 0 and "tptDrawDeviceAnimation" in msg, (what, rc, msg)
    print("refused:", what, "--", msg)
def reset():
    tpt.set_seed_mode(1); tpt.set_fold_mode(0); tpt.set_kernel_variant(0, 3, -1); tpt.set_row_shard(0, 1, 0)
refused("before any tptUpdate")
tpt.UpdateTest(0.0, 0, w, h, 3)
refused("0 frames", n=0)
refused("-1 frames", n=-1)
refused("times NULL", t=False)
refused("tile NULL", tl=False)
refused("no tptUpdate at this size", hh=h + 1)
tpt.UpdateTest(0.0, 0, 8200, 8, 3)
refused("wider than 8192", ww=8200, hh=8)
tpt.UpdateTest(0.0, 0, 8192, 8192, 3)
refused("12 GiB of colour", ww=8192, hh=8192, n=12)
tpt.UpdateTest(0.0, 0, w, h, 3)
tpt.set_row_shard(8, 2, 0); refused("row sharding"); reset()
tpt.comm_init_loopback(2, 8); refused("communicator"); tpt.comm_destroy(); reset()
mirror = np.zeros((h, w, 4), np.float32)
tpt.set_tile_mirror(mirror.ctypes.data); refused("tile mirror"); tpt.set_tile_mirror(None)
tpt.synchronize()
assert (tile == 7.25).all() and (images == -1.5).all() and list(rays) == [-5, -5, -5], "a refused call wrote a tile or a ray count"
desc = np.zeros(46 * 5, np.float32)
tpt.load_library().tptGetSceneDesc(desc.ctypes.data, None, None, None, None)
assert desc[1 * 5 + 1] == np.float32(np.cos(np.float32(0.0))) + 1 and desc[8 * 5 + 2] == 0.0, "a refused call moved the spheres"
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_through_the_host_runtime():
    out = run_refusals(REFUSALS)
    assert out.count("refused:") == 11, out
