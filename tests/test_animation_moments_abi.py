"""tptDrawDeviceAnimationMoments without a GPU: the declaration, the binding and the export of the entry point; the gfx950 code of the
clip kernels (tptTraceClipKernel: the animation kernel with the moments kernel's per-path sums) in the shipped library, held to the
queue-kernel contract relative to their twins as tests/test_animation_abi.py and tests/test_moments_abi.py state it; and the refusals,
driven through the host runtime compiled against tests/hostemu (a refused call returns before anything is enqueued)."""
import os
import re

import pytest

from isa_lib import code_object, count, exported_symbols, header_params, no_library, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import ANIM, CLIP, MOMENTS, QUEUE
from oracle_lib import ROOT

NAME = "tptDrawDeviceAnimationMoments"


def test_header_declares_the_entry_point():
    assert header_params(NAME) == ["int firstFrame", "int nFrames", "const float* times", "int screenWidth", "int screenHeight",
                                   "float* deviceTile", "float* deviceMoments", "float* deviceFrameImages", "float* deviceFrameAlbedo",
                                   "float* deviceFrameNormalDepth", "float* deviceFrameMoments", "int64_t* deviceFrameRays",
                                   "unsigned testFlags"]


def test_binding_and_export():
    from toypathtracer_amd import api
    assert NAME in api.C_ABI_SYMBOLS
    assert callable(api.draw_device_animation_moments)
    lib = api.load_library()
    assert hasattr(lib, NAME)
    assert re.search(r"\bT %s\b" % NAME, exported_symbols(api.library_path()))


@pytest.mark.parametrize("args", [
    dict(times=[[0.0, 1.0]]), dict(w=0), dict(h=-3), dict(w=8.0), dict(tile=0), dict(tile=None), dict(mo=None), dict(mo=0),
    dict(mo=1.5), dict(images="x"), dict(albedo=-16), dict(nd=2.0), dict(fm=True), dict(rays="x"),
], ids=lambda a: ",".join("%s=%r" % kv for kv in a.items()))
def test_binding_checks_arguments_before_the_library(monkeypatch, args):
    """`times` as draw_device_animation checks it, sizes and pointers as draw_device_moments checks them"""
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(times=[0.0, 0.5], w=16, h=8, tile=4096, mo=8192, images=None, albedo=None, nd=None, fm=None, rays=None)
    a.update(args)
    with pytest.raises(ValueError):
        api.draw_device_animation_moments(a["times"], 0, a["w"], a["h"], a["tile"], a["mo"], 3, images_ptr=a["images"], albedo_ptr=a["albedo"],
                                          normal_depth_ptr=a["nd"], frame_moments_ptr=a["fm"], rays_ptr=a["rays"])


# ---------------------------------------------------------------- the shipped gfx950 code
@pytest.mark.parametrize("lds", [1, 0], ids=["lds-scene", "flat-global"])
def test_clip_kernels_keep_the_queue_kernel_contract(code_object, lds):  # noqa: F811
    bodies, meta = code_object
    name = CLIP % lds
    assert name in meta and name in bodies, "the clip kernel is missing from the shipped code object"
    body, m = bodies[name], meta[name]
    assert count(body, r"flat_") == 0, "a FLAT instruction: an LDS pointer lost its address space"
    assert count(body, r"ds_(read|load)") >= 30 and count(body, r"ds_(write|store)") >= 15
    assert count(body, r"buffer_(load|store|atomic)") == 0
    assert m["agpr_count"] == 0
    assert m["vgpr_count"] <= 128, m
    assert m["max_flat_workgroup_size"] == 512 and m["wavefront_size"] == 64
    # the same matrix-core filter as its single-frame twin (8 MFMA for the <= 64-sphere table), none without the scene in LDS
    twin = QUEUE % (lds, 0)
    assert count(body, r"v_mfma") == count(bodies[twin], r"v_mfma") == (8 if lds else 0)
    # the LDS of its single-frame twin: the centres replace path records, the sums live in global memory
    assert m["group_segment_fixed_size"] == meta[twin]["group_segment_fixed_size"] == meta[ANIM % lds]["group_segment_fixed_size"]
    # spills not above the single-frame moments kernel's
    mom = meta[MOMENTS % lds]
    assert m["vgpr_spill_count"] <= mom["vgpr_spill_count"] and m["private_segment_fixed_size"] <= mom["private_segment_fixed_size"], (m, mom)
    if lds:
        assert m["vgpr_count"] <= 120, m  # (as the single-frame kernel: the resolve kernel's waves start beside it)
    # three planes per finished pixel and the moment sums: global stores beyond the animation kernel's
    assert count(body, r"global_store_dwordx4") >= count(bodies[ANIM % lds], r"global_store_dwordx4") + 3


def test_clip_kernel_takes_the_lds_of_its_twins():
    """tptQueueLdsBytes sees the centres table alone (a.moveCentres): the planes add no LDS, so the default scene keeps two workgroups per
    CU; and the per-path sums are addressed with the pool size the host sizes their buffer with"""
    csrc = os.path.join(ROOT, "toypathtracer_amd", "csrc")
    src = open(os.path.join(csrc, "tpt_queue_layout.h")).read()
    assert "if (moving) bytes += (size_t)TPT_Q_ANIM_TABLE_BYTES - (size_t)TPT_Q_NF4 * TPT_Q_ANIM_PATHS * 16;" in src
    assert "a.aovSums + kAovSums * ((size_t)(blockIdx.x + (unsigned)a.helperBase) * TPT_Q_PATHS + p)" in open(os.path.join(csrc, "tpt_kernels.hip")).read()
    assert "int tptQueuePathsPerBlock() { return TPT_Q_PATHS; }" in src
    host = open(os.path.join(csrc, "tpt_host_pipeline.cpp")).read()
    assert "(momentsBytes ? 3 : 2) * sizeof(f4) * (size_t)maxGridBlocks(P) * (size_t)tptQueuePathsPerBlock()" in host


# ---------------------------------------------------------------- refusals, through the host runtime
REFUSALS = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
w, h, n = 16, 8, 3
plane = w * h * 16
tile = np.full((h, w, 4), 7.25, np.float32)
mo = np.full((h, w, 4), 0.5, np.float32)
images = np.full((n, h, w, 4), -1.5, np.float32)
alb = np.full((n, h, w, 4), 0.25, np.float32)
nd = np.full((n, h, w, 4), 3.0, np.float32)
fmo = np.full((n, h, w, 4), -0.75, np.float32)
rays = np.full(n, -5, np.int64)
big = np.zeros((2 * n, h, w, 4), np.float32)
times = np.float32([0.0, 0.25, 0.5])
ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
F = "tptDrawDeviceAnimationMoments"
def call(ww=w, hh=h, nn=n, t=times, tl=tile, m=mo, im=images, a=alb, d=nd, fm=fmo, r=rays):
    return lib.tptDrawDeviceAnimationMoments(0, nn, ptr(t), ww, hh, ptr(tl), ptr(m), ptr(im), ptr(a), ptr(d), ptr(fm), ptr(r), 3)
def refused(what, expect=F, **kw):
    rc = call(**kw)
    msg = lib.tptGetLastError().decode()
    assert rc != 0 and expect in msg, (what, rc, msg)
    print("refused:", what, "--", msg)
def reset():
    tpt.set_seed_mode(1); tpt.set_fold_mode(0); tpt.set_kernel_variant(0, 3, -1); tpt.set_row_shard(0, 1, 0); tpt.set_samples_per_pixel(4)
refused("no context", "not initialised")
tpt.InitializeTest()
refused("before any tptUpdate")
tpt.UpdateTest(0.0, 0, w, h, 3)
# ---- what tptDrawDeviceAnimation refuses
refused("0 frames", nn=0)
refused("-1 frames", nn=-1)
refused("times NULL", t=None)
refused("tile NULL", tl=None)
refused("no tptUpdate at this size", hh=h + 1)
tpt.UpdateTest(0.0, 0, 8200, 8, 3)
refused("wider than 8192", ww=8200, hh=8)
tpt.UpdateTest(0.0, 0, 8192, 8192, 3)
refused("12 GiB of colour", ww=8192, hh=8192, nn=12)
refused("6 GiB of colour and moments (the colour alone would pass)", ww=8192, hh=8192, nn=3)
tpt.UpdateTest(0.0, 0, w, h, 3)
tpt.set_row_shard(8, 2, 0); refused("row sharding"); reset()
tpt.comm_init_loopback(2, 8); refused("communicator"); tpt.comm_destroy(); reset()
mirror = np.zeros((h, w, 4), np.float32)
tpt.set_tile_mirror(mirror.ctypes.data); refused("tile mirror"); tpt.set_tile_mirror(None)
# ---- what tptDrawDeviceMoments refuses on top
refused("moments NULL", m=None)
tpt.set_seed_mode(0); refused("row-serial seeds"); reset()
tpt.set_fold_mode(1); refused("forward fold"); reset()
for hs, persist in ((0, 1), (1, 3)):
    tpt.set_kernel_variant(hs, persist, -1); refused("variant %d/%d" % (hs, persist))
reset()
tpt.set_samples_per_pixel(2048); refused("2048 spp"); reset()
# ---- any two of the seven buffers overlapping, each at its full extent
refused("moments is the tile", m=tile)
refused("images start at the tile", im=tile)
refused("albedo is the normal / depth", a=nd)
refused("frame moments are the moments", fm=mo)
refused("frame moments are the images", fm=images)
refused("moments inside the albedo's last plane", m=alb.ctypes.data + 2 * plane + 16)
refused("the tile is the last pixel of the frame moments", tl=fmo.ctypes.data + 3 * plane - 16)
refused("normal / depth starts in the images' last plane", im=big, d=big.ctypes.data + 3 * plane - 16)
refused("the rays lie in the images", r=images.ctypes.data + plane)
refused("the albedo starts in the rays", a=rays.ctypes.data + 8 * n - 8)
tpt.synchronize()
assert (tile == 7.25).all() and (mo == 0.5).all() and (images == -1.5).all() and (alb == 0.25).all() and (nd == 3.0).all(), "a refused call wrote"
assert (fmo == -0.75).all() and list(rays) == [-5] * n and (big == 0.0).all(), "a refused call wrote"
desc = np.zeros(46 * 5, np.float32)
lib.tptGetSceneDesc(desc.ctypes.data, None, None, None, None)
assert desc[1 * 5 + 1] == np.float32(np.cos(np.float32(0.0))) + 1 and desc[8 * 5 + 2] == 0.0, "a refused call moved the spheres"
# ---- buffers that touch without sharing a byte are taken
assert call(im=big, d=big.ctypes.data + 3 * plane) == 0, lib.tptGetLastError().decode()
print("accepted: adjacent buffers")
tpt.synchronize()
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_through_the_host_runtime():
    out = run_refusals(REFUSALS)
    assert out.count("refused:") == 2 + 8 + 3 + 6 + 10, out
    assert out.count("accepted:") == 1, out
