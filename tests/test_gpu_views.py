"""tptDrawDeviceViews: several cameras of one scene traced by one launch, each view blended into its own tile -- every view held
byte for byte against the oracle rendering that camera, and against the set-camera / update / tptDrawDevice sequence it replaces."""
import ctypes as C

import numpy as np
import pytest

from common import oracle_frames
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE, FOLD_FORWARD, SEED_PER_PIXEL, SEED_ROW_SERIAL

pytestmark = pytest.mark.gpu

# {lookFrom xyz, lookAt xyz, vfov, aperture, focusDist}: different positions, fields of view, apertures and focus distances
FOUR_VIEWS = [
    [0.0, 2.0, 3.0, 0.0, 0.0, 0.0, 60.0, 0.02, 3.0],
    [3.0, 1.5, 2.0, 0.0, 0.5, 0.0, 45.0, 0.1, 3.5],
    [-2.0, 3.0, 4.0, 0.0, 0.0, -1.0, 75.0, 0.0, 4.0],
    [0.5, 0.8, -3.0, 0.0, 0.5, 0.0, 50.0, 0.05, 2.5],
]


def ring_views(n):
    out = []
    for i in range(n):
        a = 2.0 * np.pi * i / n
        out.append([4.0 * np.sin(a), 1.5 + 0.05 * i, 4.0 * np.cos(a), 0.0, 0.5, 0.0, 40.0 + i, 0.01 * (i % 4), 3.0 + 0.1 * i])
    return out


def oracle_cam(oracle, v, w, h, mitsuba=False):
    return oracle.camera(v[0:3], v[3:6], (0, 1, 0), v[6], w / h, 0.0 if mitsuba else v[7], v[8])


def draw_views(tpt, w, h, views, frames, flags=FLAG_PROGRESSIVE, time=0.0):
    """views drawn frame by frame through tptDrawDeviceViews -> (tiles [n, h, w, 4], per-frame lists of per-view rays)"""
    import torch
    n = len(views)
    tiles = torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")
    rays = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    per = []
    for f in frames:
        tpt.UpdateTest(time, f, w, h, flags)
        r0 = tpt.ray_counter_read()
        tpt.draw_device_views(time, f, w, h, views, tiles.data_ptr(), flags, rays.data_ptr())
        r1 = tpt.ray_counter_read()
        got = rays.cpu().tolist()
        assert r1 - r0 == sum(got), (f, r1 - r0, got)
        per.append(got)
    return tiles.cpu().numpy(), per


def draw_sequential(tpt, w, h, views, frames, flags=FLAG_PROGRESSIVE, time=0.0):
    """the same views as set-camera / update / tptDrawDevice per view and frame"""
    import torch
    n = len(views)
    tiles = torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    per = []
    for f in frames:
        got = []
        for v in range(n):
            p = views[v]
            tpt.set_camera(p[0:3], p[3:6], p[6], p[7], p[8])
            tpt.UpdateTest(time, f, w, h, flags)
            r0 = tpt.ray_counter_read()
            tpt.draw_device(time, f, w, h, tiles[v].data_ptr(), flags)
            got.append(tpt.ray_counter_read() - r0)
        per.append(got)
    tpt.set_camera(None)
    return tiles.cpu().numpy(), per


def check_against_oracle(oracle, tiles, per, views, w, h, spp, nframes, flags=FLAG_PROGRESSIVE, **kw):
    for v, p in enumerate(views):
        ro, bo, pero = oracle_frames(oracle, w, h, spp, nframes, flags=flags, cam=oracle_cam(oracle, p, w, h), seed_mode=SEED_PER_PIXEL, **kw)
        assert [per[f][v] for f in range(nframes)] == pero, v
        assert tiles[v].tobytes() == bo.tobytes(), "view %d differs from the oracle" % v


def test_four_cameras_equal_the_oracle(tpt_defaults, oracle):
    tpt = tpt_defaults
    w, h, spp = 200, 120, 4
    tpt.set_samples_per_pixel(spp)
    tiles, per = draw_views(tpt, w, h, FOUR_VIEWS, range(3))
    check_against_oracle(oracle, tiles, per, FOUR_VIEWS, w, h, spp, 3)
    # the launch was the views kernel with two workgroups per CU (its cameras take the LDS of the path records it gives up)
    info = tpt.launch_info()
    assert info["blocks_per_cu"] == 2, info


@pytest.mark.parametrize("mitsuba", [False, True], ids=["default", "mitsuba"])
def test_views_equal_the_sequential_calls(tpt_defaults, mitsuba):
    tpt = tpt_defaults
    w, h = 160, 96
    tpt.set_config(True, 0.9, mitsuba)
    a, pa = draw_views(tpt, w, h, FOUR_VIEWS, range(2))
    b, pb = draw_sequential(tpt, w, h, FOUR_VIEWS, range(2))
    assert pa == pb
    assert a.tobytes() == b.tobytes()


def test_one_view_is_tptDrawDevice(tpt_defaults):
    tpt = tpt_defaults
    w, h = 128, 72
    a, pa = draw_views(tpt, w, h, FOUR_VIEWS[1:2], range(3))
    b, pb = draw_sequential(tpt, w, h, FOUR_VIEWS[1:2], range(3))
    assert pa == pb and a.tobytes() == b.tobytes()


def test_thirty_two_views(tpt_defaults, oracle):
    tpt = tpt_defaults
    w, h, spp = 64, 40, 1
    views = ring_views(32)
    tpt.set_samples_per_pixel(spp)
    tiles, per = draw_views(tpt, w, h, views, range(2))
    check_against_oracle(oracle, tiles, per, views, w, h, spp, 2)


def test_ragged_size(tpt_defaults, oracle):
    tpt = tpt_defaults
    w, h, spp = 67, 41, 3
    tpt.set_samples_per_pixel(spp)
    tiles, per = draw_views(tpt, w, h, FOUR_VIEWS[:3], range(3))
    check_against_oracle(oracle, tiles, per, FOUR_VIEWS[:3], w, h, spp, 3)


def test_without_progressive_flag(tpt_defaults, oracle):
    """lerp factor 0: every tile ends up as its view's last frame alone (Test.cpp:275-276)"""
    tpt = tpt_defaults
    w, h = 96, 64
    tiles, per = draw_views(tpt, w, h, FOUR_VIEWS[1:3], range(2), flags=0)
    check_against_oracle(oracle, tiles, per, FOUR_VIEWS[1:3], w, h, 4, 2, flags=0)


def test_animated_scene(tpt_defaults, oracle):
    """kFlagAnimate: every view sees the scene of the last tptUpdate (spheres 1 and 8 moved to time 1.3)"""
    tpt = tpt_defaults
    w, h, t = 96, 64, 1.3
    flags = FLAG_PROGRESSIVE | FLAG_ANIMATE
    tiles, per = draw_views(tpt, w, h, FOUR_VIEWS[:2], range(2), flags=flags, time=t)
    check_against_oracle(oracle, tiles, per, FOUR_VIEWS[:2], w, h, 4, 2, flags=flags, time=t)


def test_grouped_scene(tpt_defaults, oracle):
    """a scene of 4096 spheres: the grouped traversal (tptTraceViewsKernel<false>)"""
    from toypathtracer_amd.scenes import stress_scene
    tpt = tpt_defaults
    s, m = stress_scene(4096, 64)
    w, h, spp = 96, 64, 2
    tpt.set_scene(s, m)
    tpt.set_samples_per_pixel(spp)
    views = [[0.0, 6.0, 20.0, 0.0, 0.0, 0.0, 60.0, 0.02, 20.0], [12.0, 4.0, 12.0, 0.0, 0.0, 0.0, 50.0, 0.0, 17.0],
             [-5.0, 10.0, 15.0, 0.0, 0.0, 2.0, 70.0, 0.05, 18.0]]
    tiles, per = draw_views(tpt, w, h, views, range(2))
    assert tpt.scene_info()["groups"] > 0
    check_against_oracle(oracle, tiles, per, views, w, h, spp, 2, spheres=s, mats=m)


def test_views_between_streamed_frames(tpt_defaults, oracle):
    """320x180: streamed tptDrawDevice frames are stream-batched; a views call in the middle drops the unserved planes, and every frame
    before and after it and every view equal the oracle (the context's camera is untouched)"""
    import torch
    tpt = tpt_defaults
    w, h = 320, 180
    views = FOUR_VIEWS[1:4]
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    vt = torch.zeros((len(views), h, w, 4), dtype=torch.float32, device="cuda")
    vr = torch.zeros((len(views),), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    r0 = tpt.ray_counter_read()
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    for f in range(4):
        tpt.draw_device(0.0, f, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
    tpt.draw_device_views(0.0, 0, w, h, views, vt.data_ptr(), FLAG_PROGRESSIVE, vr.data_ptr())
    for f in range(4, 8):
        tpt.draw_device(0.0, f, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
    rays = tpt.ray_counter_read() - r0
    ro, bo, _ = oracle_frames(oracle, w, h, 4, 8, seed_mode=SEED_PER_PIXEL)
    assert tile.cpu().numpy().tobytes() == bo.tobytes()
    got = vt.cpu().numpy()
    view_rays = vr.cpu().tolist()
    for v, p in enumerate(views):
        rv, bv, _ = oracle_frames(oracle, w, h, 4, 1, cam=oracle_cam(oracle, p, w, h), seed_mode=SEED_PER_PIXEL)
        assert view_rays[v] == rv and got[v].tobytes() == bv.tobytes(), v
    assert rays == ro + sum(view_rays)


def test_kernel_timing_counts_the_views_launch(tpt_defaults):
    import torch
    tpt = tpt_defaults
    w, h = 64, 40
    tiles = torch.zeros((2, h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    tpt.kernel_timing_begin(8)
    tpt.draw_device_views(0.0, 0, w, h, FOUR_VIEWS[:2], tiles.data_ptr(), FLAG_PROGRESSIVE)
    ms, n = tpt.kernel_timing_end()
    assert n == 1 and ms > 0.0


def test_refusals_leave_the_tiles_alone(tpt_defaults):
    import torch
    tpt = tpt_defaults

    def _reset_knobs(t):
        t.set_seed_mode(SEED_PER_PIXEL)
        t.set_fold_mode(0)
        t.set_kernel_variant(0, 3, -1)
        t.set_row_shard(0, 1, 0)

    lib = tpt.load_library()
    w, h = 64, 40
    sentinel = 7.25
    tiles = torch.full((2, h, w, 4), sentinel, dtype=torch.float32, device="cuda")
    rays = torch.full((2,), -5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    two = np.ascontiguousarray(np.array(FOUR_VIEWS[:2], np.float32))
    many = np.ascontiguousarray(np.array(ring_views(33), np.float32))

    def refused(what, ww=w, hh=h, n=2, views=two, tile_ptr=None):
        tp = tiles.data_ptr() if tile_ptr is None else tile_ptr
        rc = lib.tptDrawDeviceViews(0.0, 0, ww, hh, n, views.ctypes.data if views is not None else None, C.c_void_p(tp) if tp else None,
                                    C.c_void_p(rays.data_ptr()), FLAG_PROGRESSIVE)
        msg = lib.tptGetLastError().decode()
        assert rc != 0, what
        assert "tptDrawDeviceViews" in msg, (what, msg)

    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    refused("no views", n=0)
    refused("33 views", n=33, views=many)
    refused("views NULL", views=None)
    refused("tiles NULL", tile_ptr=0)
    refused("no tptUpdate at this size", hh=h + 1)
    tpt.UpdateTest(0.0, 0, 8200, 8, FLAG_PROGRESSIVE)
    refused("wider than 8192", ww=8200, hh=8)
    tpt.UpdateTest(0.0, 0, 8192, 8192, FLAG_PROGRESSIVE)
    five = np.ascontiguousarray(np.array(ring_views(5), np.float32))
    refused("5 GiB of colour planes", ww=8192, hh=8192, n=5, views=five)
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    tpt.set_seed_mode(SEED_ROW_SERIAL)
    refused("row-serial seeds")
    _reset_knobs(tpt)
    tpt.set_fold_mode(FOLD_FORWARD)
    refused("forward fold")
    _reset_knobs(tpt)
    for hs, persist in ((0, 1), (0, 0), (1, 3), (2, 1)):
        tpt.set_kernel_variant(hs, persist, -1)
        refused("kernel variant %d/%d" % (hs, persist))
    _reset_knobs(tpt)
    tpt.set_row_shard(8, 2, 0)
    refused("row sharding")
    _reset_knobs(tpt)
    tpt.comm_init_loopback(2, 8)
    try:
        refused("communicator")
    finally:
        tpt.comm_destroy()
    _reset_knobs(tpt)
    mirror = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tpt.set_tile_mirror(mirror.data_ptr())
    try:
        refused("tile mirror")
    finally:
        tpt.set_tile_mirror(None)
    _reset_knobs(tpt)
    tpt.synchronize()
    torch.cuda.synchronize()
    assert bool((tiles == sentinel).all()), "a refused call wrote a tile"
    assert rays.cpu().tolist() == [-5, -5]
    # ... and the context still draws views afterwards
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    tpt.draw_device_views(0.0, 0, w, h, two, tiles.data_ptr(), FLAG_PROGRESSIVE, rays.data_ptr())
    tpt.synchronize()
    assert min(rays.cpu().tolist()) > 0
