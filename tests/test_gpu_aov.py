"""tptDrawDeviceAov: one frame blended into the tile as tptDrawDevice blends it, plus the first-hit planes of its samples -- the tile, the
ray count and both planes held byte for byte against the CPU reference (tests/aov_checker.c, the oracle with each sample's first hit
captured), and against the calls it sits between."""
import ctypes as C

import numpy as np
import pytest

from aov_lib import AovChecker
from common import oracle_frames
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE, FOLD_FORWARD, SEED_PER_PIXEL, SEED_ROW_SERIAL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return AovChecker(tmp_path_factory.mktemp("aov_checker"))


def planes(h, w, fill=0.0):
    import torch
    return (torch.full((h, w, 4), fill, dtype=torch.float32, device="cuda"),
            torch.full((h, w, 4), fill, dtype=torch.float32, device="cuda"))


def draw_aov(tpt, w, h, frames, flags=FLAG_PROGRESSIVE, time=0.0, albedo=True, normal_depth=True):
    """frames drawn through tptDrawDeviceAov on one tile -> (tile, albedo or None, normalDepth or None, per-frame rays); the planes are
    the last frame's"""
    import torch
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    alb, nd = planes(h, w, float("nan"))
    torch.cuda.synchronize()
    per = []
    for f in frames:
        tpt.UpdateTest(time, f, w, h, flags)
        r0 = tpt.ray_counter_read()
        tpt.draw_device_aov(time, f, w, h, tile.data_ptr(), flags, albedo_ptr=alb.data_ptr() if albedo else None,
                            normal_depth_ptr=nd.data_ptr() if normal_depth else None)
        per.append(tpt.ray_counter_read() - r0)
    tpt.synchronize()
    return (tile.cpu().numpy(), alb.cpu().numpy() if albedo else None, nd.cpu().numpy() if normal_depth else None, per)


def check(checker, oracle, got, w, h, spp, nframes, **kw):
    tile, alb, nd, per = got
    pero, bo, ao, no = checker.frames(oracle, w, h, spp, nframes, **kw)
    assert per == pero
    assert tile.tobytes() == bo.tobytes(), "the tile differs from the checker"
    assert alb.tobytes() == ao.tobytes(), "the albedo plane differs from the checker"
    assert nd.tobytes() == no.tobytes(), "the normal / depth plane differs from the checker"
    return ao, no


def test_1280x720x4_equals_the_checker(tpt_defaults, checker, oracle):
    tpt = tpt_defaults
    w, h = 1280, 720
    got = draw_aov(tpt, w, h, [0])
    ao, no = check(checker, oracle, got, w, h, 4, 1)
    cov = ao[..., 3]
    assert (cov == 1).any() and (cov == 0).any()  # (hits and sky in the frame: the planes are not trivially equal)
    # the launch was the AOV kernel with the plain kernel's LDS: two workgroups per CU
    info = tpt.launch_info()
    assert info["blocks_per_cu"] == 2, info


@pytest.mark.parametrize("spp", [1, 16])
def test_ragged_size(tpt_defaults, checker, oracle, spp):
    tpt = tpt_defaults
    w, h = 333, 171
    tpt.set_samples_per_pixel(spp)
    check(checker, oracle, draw_aov(tpt, w, h, [0]), w, h, spp, 1)


def test_mitsuba_compare(tpt_defaults, checker, oracle):
    tpt = tpt_defaults
    w, h = 200, 120
    tpt.set_config(True, 0.9, True)
    cam = oracle.camera((0, 2, 3), (0, 0, 0), (0, 1, 0), 60.0, w / h, 0.0, 3.0)  # (aperture 0, Test.cpp:312-313)
    check(checker, oracle, draw_aov(tpt, w, h, [0]), w, h, 4, 1, cam=cam, mitsuba_compare=True)


def test_no_light_sampling(tpt_defaults, checker, oracle):
    tpt = tpt_defaults
    w, h = 200, 120
    tpt.set_config(False, 0.9, False)
    check(checker, oracle, draw_aov(tpt, w, h, [0]), w, h, 4, 1, light_sampling=False)


def test_animated_scene(tpt_defaults, checker, oracle):
    """tptUpdate(1.7, kFlagAnimate): the planes see spheres 1 and 8 where the colour sees them"""
    tpt = tpt_defaults
    w, h = 160, 96
    flags = FLAG_PROGRESSIVE | FLAG_ANIMATE
    check(checker, oracle, draw_aov(tpt, w, h, [0], flags=flags, time=1.7), w, h, 4, 1, flags=flags, time=1.7)


def test_grouped_scene(tpt_defaults, checker, oracle):
    """a scene of 4096 spheres: the grouped traversal (tptTraceAovKernel<false>)"""
    from toypathtracer_amd.scenes import stress_scene
    tpt = tpt_defaults
    s, m = stress_scene(4096, 64)
    w, h, spp = 96, 64, 2
    tpt.set_scene(s, m)
    tpt.set_samples_per_pixel(spp)
    tpt.set_camera((0.0, 6.0, 20.0), (0.0, 0.0, 0.0), 60.0, 0.02, 20.0)
    got = draw_aov(tpt, w, h, [0])
    assert tpt.scene_info()["groups"] > 0
    cam = oracle.camera((0.0, 6.0, 20.0), (0.0, 0.0, 0.0), (0, 1, 0), 60.0, w / h, 0.02, 20.0)
    check(checker, oracle, got, w, h, spp, 1, spheres=s, mats=m, cam=cam)


def test_tile_is_tptDrawDevice_over_three_frames(tpt_defaults, checker, oracle):
    import torch
    tpt = tpt_defaults
    w, h = 256, 144
    a = draw_aov(tpt, w, h, range(3))
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    per = []
    for f in range(3):
        tpt.UpdateTest(0.0, f, w, h, FLAG_PROGRESSIVE)
        r0 = tpt.ray_counter_read()
        tpt.draw_device(0.0, f, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
        per.append(tpt.ray_counter_read() - r0)
    assert a[3] == per
    assert a[0].tobytes() == tile.cpu().numpy().tobytes()
    # ... and the planes of the last call are frame 2's alone (overwritten, not blended)
    check(checker, oracle, a, w, h, 4, 3)


@pytest.mark.parametrize("which", ["albedo", "normal_depth"])
def test_one_plane(tpt_defaults, which):
    tpt = tpt_defaults
    w, h = 150, 90
    both = draw_aov(tpt, w, h, [0])
    one = draw_aov(tpt, w, h, [0], albedo=which == "albedo", normal_depth=which == "normal_depth")
    assert one[3] == both[3] and one[0].tobytes() == both[0].tobytes()
    k = 1 if which == "albedo" else 2
    assert one[k].tobytes() == both[k].tobytes()
    assert one[3 - k] is None


def test_aov_between_streamed_frames(tpt_defaults, checker, oracle):
    """320x180: streamed tptDrawDevice frames are stream-batched; an AOV call in the middle drops the unserved planes, and every frame
    before and after it equals the oracle, with the rays of all three kinds of frame accounted for"""
    import torch
    tpt = tpt_defaults
    w, h = 320, 180
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    at = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    alb, nd = planes(h, w, float("nan"))
    torch.cuda.synchronize()
    r0 = tpt.ray_counter_read()
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    for f in range(4):
        tpt.draw_device(0.0, f, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
    tpt.draw_device_aov(0.0, 0, w, h, at.data_ptr(), FLAG_PROGRESSIVE, albedo_ptr=alb.data_ptr(), normal_depth_ptr=nd.data_ptr())
    for f in range(4, 8):
        tpt.draw_device(0.0, f, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
    rays = tpt.ray_counter_read() - r0
    ro, bo, _ = oracle_frames(oracle, w, h, 4, 8, seed_mode=SEED_PER_PIXEL)
    assert tile.cpu().numpy().tobytes() == bo.tobytes()
    pa, ba, aa, na = checker.frames(oracle, w, h, 4, 1)
    assert at.cpu().numpy().tobytes() == ba.tobytes()
    assert alb.cpu().numpy().tobytes() == aa.tobytes() and nd.cpu().numpy().tobytes() == na.tobytes()
    assert rays == ro + pa[0]


def test_ordered_on_the_context_stream(tpt_defaults, checker, oracle):
    """the planes are filled with NaN on the context stream (behind a delay) just before the call: the call's writes come after the fill;
    a copy enqueued on the stream after the call sees the planes"""
    import torch
    tpt = tpt_defaults
    w, h = 320, 180
    stream = torch.cuda.Stream()
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    alb, nd = planes(h, w, 0.0)
    stream.wait_stream(torch.cuda.current_stream())  # (the allocations' own stream: ordering it is the host's job)
    tpt.set_stream(stream.cuda_stream)
    try:
        tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
        with torch.cuda.stream(stream):
            if hasattr(torch.cuda, "_sleep"):
                torch.cuda._sleep(50_000_000)  # (tens of ms: a trace not ordered behind the fill would finish first)
            alb.fill_(float("nan"))
            nd.fill_(float("nan"))
            tpt.draw_device_aov(0.0, 0, w, h, tile.data_ptr(), FLAG_PROGRESSIVE, albedo_ptr=alb.data_ptr(), normal_depth_ptr=nd.data_ptr())
            alb2, nd2 = alb.clone(), nd.clone()  # stream-ordered behind the call
        stream.synchronize()
    finally:
        tpt.set_stream(None)
    _, bb, ao, no = checker.frames(oracle, w, h, 4, 1)
    assert tile.cpu().numpy().tobytes() == bb.tobytes()
    assert alb2.cpu().numpy().tobytes() == ao.tobytes() and nd2.cpu().numpy().tobytes() == no.tobytes()
    assert alb.cpu().numpy().tobytes() == ao.tobytes() and nd.cpu().numpy().tobytes() == no.tobytes()


def test_refusals_leave_the_tile_and_planes_alone(tpt_defaults):
    import torch
    tpt = tpt_defaults

    def reset(t):
        t.set_seed_mode(SEED_PER_PIXEL)
        t.set_fold_mode(0)
        t.set_kernel_variant(0, 3, -1)
        t.set_row_shard(0, 1, 0)
        t.set_samples_per_pixel(4)

    lib = tpt.load_library()
    w, h = 64, 40
    tile = torch.full((h, w, 4), 7.25, dtype=torch.float32, device="cuda")
    alb = torch.full((h, w, 4), -3.5, dtype=torch.float32, device="cuda")
    nd = torch.full((h, w, 4), 11.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def refused(what, ww=w, hh=h, t=True, a=True, n=True):
        rc = lib.tptDrawDeviceAov(0.0, 0, ww, hh, C.c_void_p(tile.data_ptr()) if t else None, C.c_void_p(alb.data_ptr()) if a else None,
                                  C.c_void_p(nd.data_ptr()) if n else None, FLAG_PROGRESSIVE)
        msg = lib.tptGetLastError().decode()
        assert rc != 0, what
        assert "tptDrawDeviceAov" in msg, (what, msg)

    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    refused("both planes NULL", a=False, n=False)
    refused("tile NULL", t=False)
    refused("no tptUpdate at this size", hh=h + 1)
    tpt.UpdateTest(0.0, 0, 8200, 8, FLAG_PROGRESSIVE)
    refused("wider than 8192", ww=8200, hh=8)
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    tpt.set_seed_mode(SEED_ROW_SERIAL)
    refused("row-serial seeds")
    reset(tpt)
    tpt.set_fold_mode(FOLD_FORWARD)
    refused("forward fold")
    reset(tpt)
    for hs, persist in ((0, 1), (0, 0), (1, 3), (2, 1)):
        tpt.set_kernel_variant(hs, persist, -1)
        refused("kernel variant %d/%d" % (hs, persist))
    reset(tpt)
    tpt.set_samples_per_pixel(2048)
    refused("2048 spp")
    reset(tpt)
    tpt.set_row_shard(8, 2, 0)
    refused("row sharding")
    reset(tpt)
    tpt.comm_init_loopback(2, 8)
    try:
        refused("communicator")
    finally:
        tpt.comm_destroy()
    reset(tpt)
    mirror = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tpt.set_tile_mirror(mirror.data_ptr())
    try:
        refused("tile mirror")
    finally:
        tpt.set_tile_mirror(None)
    reset(tpt)
    tpt.synchronize()
    torch.cuda.synchronize()
    assert bool((tile == 7.25).all()) and bool((alb == -3.5).all()) and bool((nd == 11.0).all()), "a refused call wrote the tile or a plane"
    # ... and the context still draws planes afterwards
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    tpt.draw_device_aov(0.0, 0, w, h, tile.data_ptr(), FLAG_PROGRESSIVE, albedo_ptr=alb.data_ptr(), normal_depth_ptr=nd.data_ptr())
    tpt.synchronize()
    assert bool((alb[..., 3] >= 0).all()) and bool((alb[..., 3] <= 1).all())
