"""tptDrawDeviceCameraClip without a GPU: the declaration, the binding and the export of the entry point; the binding's argument checks;
the gfx950 code of the camera-clip kernels (tptCameraClipKernel: the clip kernel with a camera per frame read from the LDS camera table)
in the shipped library, held to the queue-kernel contract and to the register ceilings of the planes kernels; tptQueueVariant and
tptQueueLdsBytes compiled for the host; and the refusals, driven through the host runtime compiled against tests/hostemu (a refused call
returns before anything is enqueued)."""
import os
import re
import subprocess

import pytest

from isa_lib import code_object, count, exported_symbols, header_params, no_library, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import CAMERA_CLIP, CLIP, QUEUE, family
from oracle_lib import ROOT

NAME = "tptDrawDeviceCameraClip"


def test_header_declares_the_entry_point():
    assert header_params(NAME) == ["int firstFrame", "int nFrames", "const float* times", "const float* views", "int screenWidth",
                                   "int screenHeight", "float* deviceTile", "float* deviceMoments", "float* deviceFrameImages",
                                   "float* deviceFrameAlbedo", "float* deviceFrameNormalDepth", "float* deviceFrameMoments",
                                   "int64_t* deviceFrameRays", "void* outCameras", "unsigned testFlags"]


def test_binding_and_export():
    from toypathtracer_amd import api
    assert NAME in api.C_ABI_SYMBOLS
    assert callable(api.draw_device_camera_clip)
    lib = api.load_library()
    assert hasattr(lib, NAME)
    assert re.search(r"\bT %s\b" % NAME, exported_symbols(api.library_path()))


VIEW = [0.0, 2.0, 3.0, 0.0, 0.0, 0.0, 60.0, 0.02, 3.0]


def np_shape(v):
    import numpy as np
    return np.asarray(v).shape


@pytest.mark.parametrize("args", [
    dict(times=[[0.0, 1.0]]), dict(views=VIEW), dict(views=[VIEW]), dict(views=[VIEW] * 3), dict(views=[VIEW[:8]] * 2),
    dict(views=[[VIEW, VIEW]]), dict(times=[], views=[VIEW]), dict(w=0), dict(h=-3), dict(w=8.0), dict(tile=0), dict(tile=None),
    dict(mo=None), dict(mo=0), dict(mo=1.5), dict(images="x"), dict(albedo=-16), dict(nd=2.0), dict(fm=True), dict(rays="x"),
], ids=lambda a: ",".join("%s=%r" % (k, v if k != "views" else np_shape(v)) for k, v in a.items()))
def test_binding_checks_arguments_before_the_library(monkeypatch, args):
    """`times` and the sizes and pointers as draw_device_animation_moments checks them; `views` (N, 9) with N = len(times)"""
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(times=[0.0, 0.5], views=[VIEW, VIEW], w=16, h=8, tile=4096, mo=8192, images=None, albedo=None, nd=None, fm=None, rays=None)
    a.update(args)
    with pytest.raises(ValueError):
        api.draw_device_camera_clip(a["times"], a["views"], 0, a["w"], a["h"], a["tile"], a["mo"], 3, images_ptr=a["images"],
                                    albedo_ptr=a["albedo"], normal_depth_ptr=a["nd"], frame_moments_ptr=a["fm"], rays_ptr=a["rays"])


# ---------------------------------------------------------------- the shipped gfx950 code
@pytest.mark.parametrize("lds", [1, 0], ids=["lds-scene", "flat-global"])
def test_camera_clip_kernels_keep_the_queue_kernel_contract(code_object, lds):  # noqa: F811
    bodies, meta = code_object
    name = CAMERA_CLIP % lds
    assert name in meta and name in bodies, "the camera-clip kernel is missing from the shipped code object"
    body, m = bodies[name], meta[name]
    assert count(body, r"flat_") == 0, "a FLAT instruction: an LDS pointer lost its address space"
    assert count(body, r"buffer_(load|store|atomic)") == 0
    assert m["agpr_count"] == 0
    assert m["max_flat_workgroup_size"] == 512 and m["wavefront_size"] == 64
    # the matrix-core filter of its single-frame twin (8 MFMA for the <= 64-sphere table), none without the scene in LDS
    twin = QUEUE % (lds, 0)
    assert count(body, r"v_mfma") == count(bodies[twin], r"v_mfma") == (8 if lds else 0)
    # the LDS of its single-frame twin: both tables replace path records, the sums live in global memory
    assert m["group_segment_fixed_size"] == meta[twin]["group_segment_fixed_size"] == meta[CLIP % lds]["group_segment_fixed_size"]
    # the ceiling: what the project ships for a planes kernel (128 VGPRs / 6 spilled / 28 B of scratch); with the scene in LDS 120
    # VGPRs, so that the resolve kernel's waves start beside it
    assert m["vgpr_count"] <= (120 if lds else 128), m
    assert m["vgpr_spill_count"] <= 6 and m["private_segment_fixed_size"] <= 28, m
    # every plane store of the clip kernel
    assert count(body, r"global_store_dwordx4") >= count(bodies[CLIP % lds], r"global_store_dwordx4")


def test_exactly_one_new_kernel_pair(code_object):  # noqa: F811
    _, meta = code_object
    assert sorted(n for n in meta if "CameraClip" in n) == sorted(family(CAMERA_CLIP))


# ---------------------------------------------------------------- the variant decision and the LDS of a launch, on the host
VARIANT_PROGRAM = r'''
#include <cstdio>
#include <initializer_list>
#include "tpt_queue_layout.h"
using namespace tpt;
int main()
{
    static CameraPOD cams[32];
    static f4 centres[64], sums[3], plane[1];
    KernelArgs a{};
    a.scene.nPairs = 23; a.scene.nSpheres = 46; a.scene.nLights = 2; a.scene.mxR1 = 0; // (the built-in scene)
    a.batchFrames = 1;
    const size_t single = tptQueueLdsBytes(a, true), singleFlat = tptQueueLdsBytes(a, false);
    printf("single %d\n", (int)tptQueueVariant(a));
    a.batchFrames = 32;
    a.viewCams = cams; a.moveCentres = centres; a.aovSums = sums; a.momentsOut = plane;
    printf("both %d %d\n", (int)tptQueueVariant(a), (int)QV_CAMERA_CLIP);
    printf("lds %zu %zu %zu %zu\n", tptQueueLdsBytes(a, true), single, tptQueueLdsBytes(a, false), singleFlat);
    printf("two_per_cu %d\n", (int)(160 * 1024 / (tptQueueLdsBytes(a, true) + 256)));
    for (int n : {1, 17}) { a.batchFrames = n; printf("frames %d %d\n", n, (int)tptQueueVariant(a)); }
    for (int n : {0, 33}) { a.batchFrames = n; printf("invalid frames %d %d\n", n, (int)(tptQueueVariant(a) == QV_INVALID)); }
    a.batchFrames = 32;
    a.momentsOut = nullptr; printf("invalid no-moments %d\n", (int)(tptQueueVariant(a) == QV_INVALID)); a.momentsOut = plane;
    a.aovSums = nullptr; printf("invalid no-sums %d\n", (int)(tptQueueVariant(a) == QV_INVALID));
    a.momentsOut = nullptr; printf("invalid no-planes %d\n", (int)(tptQueueVariant(a) == QV_INVALID));
    a.aovSums = sums; a.momentsOut = plane;
    a.scene.nGroups = 4; printf("invalid grouped %d\n", (int)(tptQueueVariant(a) == QV_INVALID)); a.scene.nGroups = 0;
    a.moveCentres = nullptr; a.aovSums = nullptr; a.momentsOut = nullptr; printf("views %d\n", (int)(tptQueueVariant(a) == QV_VIEWS));
    a.viewCams = nullptr; a.moveCentres = centres; a.aovSums = sums; a.momentsOut = plane; printf("clip %d\n", (int)(tptQueueVariant(a) == QV_CLIP));
    printf("last %d\n", (int)(QV_CAMERA_CLIP + 1 == QV_INVALID));
    return 0;
}
'''


def test_variant_and_lds_on_the_host(tmp_path):
    src, exe = str(tmp_path / "variant.cpp"), str(tmp_path / "variant")
    open(src, "w").write(VARIANT_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-include", "hip/hip_runtime.h",
                           "-I", os.path.join(ROOT, "tests", "hostemu"), "-I", os.path.join(ROOT, "toypathtracer_amd", "csrc"), src, "-o", exe])
    out = dict(ln.rsplit(" ", 1) if not ln.startswith(("both", "lds")) else (ln.split()[0], ln.split()[1:])
               for ln in subprocess.check_output([exe]).decode().splitlines())
    assert out["both"][0] == out["both"][1], "both tables with the planes select the camera-clip variant"
    assert out["frames 1"] == out["frames 17"] == out["both"][0]
    for case in ("frames 0", "frames 33", "no-moments", "no-sums", "no-planes", "grouped"):
        assert out["invalid " + case] == "1", case
    assert out["views"] == "1" and out["clip"] == "1", "the existing decisions stand"
    assert out["last"] == "1", "the new enumerator sits right before QV_INVALID"
    lds, single, flat, single_flat = (int(v) for v in out["lds"])
    assert lds == single and flat == single_flat, "the LDS of a launch is its single-frame twin's"
    assert out["two_per_cu"] == "2"


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
cams = np.full(12 * 88, 0xA5, np.uint8)
times = np.float32([0.0, 0.25, 0.5])
views = np.float32([[3.0 * np.sin(0.1 * j), 2.0, 3.0 * np.cos(0.1 * j), 0.0, 0.0, 0.0, 50.0, 0.05, 2.5] for j in range(12)])
ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
F = "tptDrawDeviceCameraClip"
def call(ww=w, hh=h, nn=n, t=times, v=views, tl=tile, m=mo, im=images, a=alb, d=nd, fm=fmo, r=rays, c=cams):
    return lib.tptDrawDeviceCameraClip(0, nn, ptr(t), ptr(v), ww, hh, ptr(tl), ptr(m), ptr(im), ptr(a), ptr(d), ptr(fm), ptr(r), ptr(c), 3)
def scene_desc():
    s, cam = np.zeros(46 * 5, np.float32), np.zeros(22, np.float32)
    lib.tptGetSceneDesc(s.ctypes.data, None, cam.ctypes.data, None, None)
    return s.tobytes() + cam.tobytes()
state = None
def refused(what, expect=F, **kw):
    rc = call(**kw)
    msg = lib.tptGetLastError().decode()
    assert rc != 0 and expect in msg, (what, rc, msg)
    assert (cams == 0xA5).all(), (what, "outCameras written")
    assert state is None or scene_desc() == state, (what, "the camera or the spheres changed")
    print("refused:", what, "--", msg)
def reset():
    tpt.set_seed_mode(1); tpt.set_fold_mode(0); tpt.set_kernel_variant(0, 3, -1); tpt.set_row_shard(0, 1, 0); tpt.set_samples_per_pixel(4)
def update(ww, hh):
    global state
    tpt.UpdateTest(0.0, 0, ww, hh, 3)
    state = scene_desc()
refused("no context", "not initialised")
tpt.InitializeTest()
refused("before any tptUpdate")
update(w, h)
# ---- what tptDrawDeviceAnimation refuses
refused("0 frames", nn=0)
refused("-1 frames", nn=-1)
refused("times NULL", t=None)
refused("tile NULL", tl=None)
refused("no tptUpdate at this size", hh=h + 1)
update(8200, 8)
refused("wider than 8192", ww=8200, hh=8)
update(8192, 8192)
refused("12 GiB of colour", ww=8192, hh=8192, nn=12)
refused("6 GiB of colour and moments (the colour alone would pass)", ww=8192, hh=8192, nn=3)
update(w, h)
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
# ---- its own
refused("views NULL", v=None)
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
assert (fmo == -0.75).all() and list(rays) == [-5] * n and (big == 0.0).all() and (cams == 0xA5).all(), "a refused call wrote"
desc = np.zeros(46 * 5, np.float32)
lib.tptGetSceneDesc(desc.ctypes.data, None, None, None, None)
assert desc[1 * 5 + 1] == np.float32(np.cos(np.float32(0.0))) + 1 and desc[8 * 5 + 2] == 0.0, "a refused call moved the spheres"
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_through_the_host_runtime():
    out = run_refusals(REFUSALS)
    assert out.count("refused:") == 2 + 8 + 3 + 6 + 1 + 10, out
