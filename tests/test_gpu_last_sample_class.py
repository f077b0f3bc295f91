"""The seventh class of the frame-pools kernel for scenes staged in LDS (csrc/tpt_queue_layout.h, Q_LAST): an ended sample goes to END when its pixel has a further
sample and to LAST when it was the pixel's last one; a LAST batch stores its pixels and starts the next pixels in the same lanes.  Which
path and lane serve a pixel changes, a pixel's arithmetic and its random numbers do not: tptDrawDeviceBatch of k frames must leave the
bytes and count the rays of k tptDrawDevice calls, one launch each -- the single-frame kernel, which has no such class --, and frame 0
of those must be the oracle's.

Sizes: 200x120 has several chunks per workgroup and a width that is no multiple of 8.  16x8 has fewer pixels than one workgroup has
paths; its launches have too few workgroups for a pool per frame (fewer than two per frame: csrc/tpt_frame_pools.h) and take the shared
pool's kernel, which the case pins as it is.  32x32 is the smallest frame whose batches DO take a pool per frame (16 chunks, two
workgroups per frame): a workgroup serves at most its frame's 1024 pixels with 920 paths, so its LAST batches find no pixel left -- start
and drain only."""
import numpy as np
import pytest

from oracle_lib import FLAG_PROGRESSIVE, SEED_PER_PIXEL

pytestmark = pytest.mark.gpu

FRAMES = 11  # the longest run of frames a case asks for (the stream below)
_SINGLE = {}


def scene_of(name):
    """-> ((spheres, materials) or None for the built-in scene, camera knobs or None)"""
    if name == "default":
        return None, None
    if name == "lights16":  # 16 emissive spheres: eight times the built-in scene's light list in the workgroup's LDS, and 16 shadow rays per Lambert hit
        from lights_lib import default_with_lights
        return default_with_lights(16), None
    assert name == "grouped256"  # 256 spheres in groups: tptFramePoolsKernel<false>, which keeps one END class
    from toypathtracer_amd.scenes import STRESS_CAMERA, stress_scene
    return stress_scene(256, 16), STRESS_CAMERA


def set_up(tpt, name, spp):
    scene, cam = scene_of(name)
    if scene is not None:
        tpt.set_scene(*scene)
    if cam is not None:
        tpt.set_camera(**cam)
    tpt.set_samples_per_pixel(spp)
    tpt.set_host_lookahead(0)  # (frames this small may be blended before the next call arrives: the caller must not look synchronous)


def single_frames(tpt, oracle, name, w, h, spp):
    """FRAMES tptDrawDevice calls on a zeroed tile, one launch and one wait each (tptSetStreamBatching off), once per scene and shape:
    (every frame's rays, the tile bytes after every frame).  Shared by the cases, never modified.  Frame 0 is held against the oracle."""
    import torch
    key = (name, w, h, spp)
    if key not in _SINGLE:
        set_up(tpt, name, spp)
        tpt.set_stream_batching(False)
        tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        per, tiles = [], []
        for f in range(FRAMES):
            r0 = tpt.ray_counter_read()
            tpt.UpdateTest(0.0, f, w, h, FLAG_PROGRESSIVE)
            tpt.draw_device(0.0, f, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
            tpt.synchronize()
            per.append(tpt.ray_counter_read() - r0)
            tiles.append(tile.cpu().numpy().tobytes())
        tpt.set_stream_batching(True)
        scene, cam = scene_of(name)
        spheres, mats = scene if scene is not None else oracle.default_scene()
        c = oracle.default_camera(w, h) if cam is None else oracle.camera(cam["look_from"], cam["look_at"], (0, 1, 0), cam["vfov"], w / h, cam["aperture"], cam["focus_dist"])
        bb = np.zeros((h, w, 4), np.float32)
        r, _ = oracle.render(spheres, mats, c, w, h, spp, 0, FLAG_PROGRESSIVE, backbuffer=bb, seed_mode=SEED_PER_PIXEL)
        assert per[0] == r and tiles[0] == bb.tobytes(), "frame 0 of the single-frame kernel differs from the oracle"
        _SINGLE[key] = (per, tiles)
    return _SINGLE[key]


def batch_equals_singles(tpt, oracle, name, w, h, spp, k):
    import torch
    per, tiles = single_frames(tpt, oracle, name, w, h, spp)
    set_up(tpt, name, spp)
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r0 = tpt.ray_counter_read()
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    tpt.draw_device_batch(0.0, 0, k, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
    tpt.synchronize()
    rays = tpt.ray_counter_read() - r0
    grid = tpt.launch_info()["grid_blocks"]
    print("last-sample class %s %dx%dx%d k=%d: grid %d (%s), rays %d, single frames %s" % (
        name, w, h, spp, k, grid, "a pool per frame" if grid >= 2 * k else "shared pool", rays, per[:k]))
    assert rays == sum(per[:k])
    assert tile.cpu().numpy().tobytes() == tiles[k - 1]
    return grid


SIZES = [(16, 8), (200, 120), (32, 32)]


@pytest.mark.parametrize("k", [2, 5, 8])
@pytest.mark.parametrize("spp", [1, 2, 4, 5])
@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_batch_equals_single_frame_launches(tpt_defaults, oracle, w, h, spp, k):
    grid = batch_equals_singles(tpt_defaults, oracle, "default", w, h, spp, k)
    assert (grid >= 2 * k) == ((w, h) != (16, 8)), "the kernel this size is here for (csrc/tpt_frame_pools.h, framePoolsOfLaunch)"


@pytest.mark.parametrize("spp,k", [(1, 5), (4, 5)])
def test_sixteen_lights(tpt_defaults, oracle, spp, k):
    assert batch_equals_singles(tpt_defaults, oracle, "lights16", 200, 120, spp, k) >= 2 * k


@pytest.mark.parametrize("spp", [1, 4])
def test_grouped_scene(tpt_defaults, oracle, spp):
    tpt = tpt_defaults
    assert batch_equals_singles(tpt, oracle, "grouped256", 64, 36, spp, 2) >= 4
    assert tpt.scene_info()["groups"] > 0  # (tptFramePoolsKernel<false>)


def _stream(tpt, tile, w, h, frames):
    """consecutive tptDrawDevice calls without a wait -> trace launches made for them"""
    tpt.kernel_timing_begin(len(frames) + 1)
    for f in frames:
        tpt.UpdateTest(0.0, f, w, h, FLAG_PROGRESSIVE)
        tpt.draw_device(0.0, f, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
    return tpt.kernel_timing_end()[1]


@pytest.mark.parametrize("spp", [1, 4])
def test_stream_launch_counts_every_frame(tpt_hooks, oracle, spp):
    """tptDrawDeviceBatch adds its frames' rays to one total; a STREAM launch of the same kernel keeps a counter per frame (the hooks
    build reads them): 10 calls, frames 2 .. 9 in one launch of 8, every frame's count the single-frame launch's."""
    import torch
    tpt = tpt_hooks
    w, h = 200, 120
    per, tiles = single_frames(tpt, oracle, "default", w, h, spp)
    set_up(tpt, "default", spp)
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert _stream(tpt, tile, w, h, range(0, 10)) == 3, "the stream rule no longer batches this shape 8 to a launch"
    tpt.synchronize()
    assert tpt.test_stream_frame_rays() == per[2:10]
    assert tile.cpu().numpy().tobytes() == tiles[9]


@pytest.mark.parametrize("spp", [1, 4])
def test_cut_stream_equals_single_frame_launches(tpt_defaults, oracle, spp):
    """11 tptDrawDevice calls: frames 0 and 1 go out alone, frame 2 starts a launch of 8 frames with a pool per frame, and the caller
    waits after frame 4, the third of that launch -- the launch is cut, workgroups of the unasked frames serve the asked ones.  Exact at
    that wait and at the end, against the same frames drawn one launch each."""
    import torch
    tpt = tpt_defaults
    w, h = 200, 120
    per, tiles = single_frames(tpt, oracle, "default", w, h, spp)
    set_up(tpt, "default", spp)
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r0 = tpt.ray_counter_read()
    assert _stream(tpt, tile, w, h, range(0, 5)) == 3, "the stream rule no longer batches this shape"
    assert tpt.launch_info()["grid_blocks"] >= 16  # (a pool per frame)
    tpt.synchronize()
    assert tpt.ray_counter_read() - r0 == sum(per[:5])
    assert tile.cpu().numpy().tobytes() == tiles[4]
    _stream(tpt, tile, w, h, range(5, FRAMES))
    tpt.synchronize()
    assert tpt.ray_counter_read() - r0 == sum(per[:FRAMES])
    assert tile.cpu().numpy().tobytes() == tiles[FRAMES - 1]
