"""tptDrawDeviceCameraClip on the GPU: the frames of a clip whose camera moves, each with its denoiser planes, up to 32 per launch.  Every
frame's image, albedo, normal / depth, moments plane, ray count and Camera record, the final tile and the final moments are held byte
for byte (no tolerance anywhere) against the tptSetCamera + tptUpdate + tptDrawDeviceMoments sequence the call replaces and against the
CPU statement of the trace (tests/moments_checker.c) with each view's camera and the spheres moved to each time; then the clip in which
nothing moves, the scenes that go frame by frame, the optional outputs, the context afterwards and the temporal pass on the call's
planes and cameras."""
import numpy as np
import pytest

from moments_lib import MomentsChecker
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE
from test_gpu_animation import irregular_times
from test_gpu_animation_moments import GUARD, OUTPUTS, assert_same, draw_clip, guarded, guards_intact, previous, same

pytestmark = pytest.mark.gpu

ANIMATED = FLAG_PROGRESSIVE | FLAG_ANIMATE
STEP = 5.0  # degrees of orbit per frame


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return MomentsChecker(tmp_path_factory.mktemp("moments_checker"))


def orbit_views(n, step=STEP, height=2.0, radius=3.0, focus=3.0):
    """the default camera (Test.cpp:309-319) carried round its look-at, `step` degrees per frame about the y axis"""
    out = []
    for j in range(n):
        a = np.radians(step * j)
        out.append([radius * np.sin(a), height, radius * np.cos(a), 0.0, 0.0, 0.0, 60.0, 0.02, focus])
    return np.asarray(out, np.float32)


def oracle_cam(oracle, v, w, h, mitsuba=False):
    return oracle.camera(v[0:3], v[3:6], (0, 1, 0), v[6], w / h, 0.0 if mitsuba else v[7], v[8])


def draw_camera_clip(tpt, w, h, times, views, first=0, flags=ANIMATED, outputs=OUTPUTS, prev=None, cameras=True):
    """one tptDrawDeviceCameraClip call on a tile and a moments plane with previous contents -> dict of device tensors: tile, moments,
    the requested per-frame outputs ([n, h, w, 4]; untouched sentinel planes for those not requested), rays (a list) and cams.  Guard
    planes around every buffer are checked."""
    import torch
    n = len(times)
    tile0, mo0 = prev if prev is not None else previous(w, h)
    tile, mo = guarded(1, h, w, tile0[None]), guarded(1, h, w, mo0[None])
    per = {k: guarded(n, h, w) for k in OUTPUTS[:4]}
    rays = torch.full((n + 2,), -9, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    tpt.UpdateTest(times[0], first, w, h, flags)  # (the call refuses a size no tptUpdate has seen)
    r0 = tpt.ray_counter_read()
    ptr = lambda k: per[k][1].data_ptr() if k in outputs else None  # noqa: E731
    cams = tpt.draw_device_camera_clip(times, views, first, w, h, tile[1].data_ptr(), mo[1].data_ptr(), flags, images_ptr=ptr("images"),
                                       albedo_ptr=ptr("albedo"), normal_depth_ptr=ptr("nd"), frame_moments_ptr=ptr("fmo"),
                                       rays_ptr=rays[1:].data_ptr() if "rays" in outputs else None, cameras=cameras)
    total = tpt.ray_counter_read() - r0
    torch.cuda.synchronize()
    for name, t in list(per.items()) + [("tile", tile), ("moments", mo)]:
        assert guards_intact(t), "the call wrote outside %s" % name
        if name in OUTPUTS and name not in outputs:
            assert bool((t == GUARD).all()), "the call wrote %s, which was not requested" % name
    r = rays.cpu().tolist()
    assert r[0] == -9 and r[-1] == -9
    if "rays" in outputs:
        assert total == sum(r[1:-1]), (total, r)
    else:
        assert r == [-9] * (n + 2)
    assert (cams is None) == (not cameras)
    out = {k: per[k][1:n + 1] for k in per}
    out.update(tile=tile[1], moments=mo[1], rays=r[1:-1], total=total, cams=cams)
    return out


def draw_camera_sequence(tpt, w, h, times, views, first=0, flags=ANIMATED, prev=None):
    """the same frames as tptSetCamera + tptUpdate + tptDrawDeviceMoments per frame on buffers with the same previous contents, the tile
    and the moments read after each frame, the camera taken from tptGetSceneDesc after each tptUpdate -> the same dict"""
    import torch
    n = len(times)
    tile0, mo0 = prev if prev is not None else previous(w, h)
    tile, mo = torch.from_numpy(tile0).cuda(), torch.from_numpy(mo0).cuda()
    out = {k: torch.full((n, h, w, 4), GUARD, dtype=torch.float32, device="cuda") for k in OUTPUTS[:4]}
    torch.cuda.synchronize()
    rays, cams = [], []
    for j, t in enumerate(times):
        v = [float(x) for x in views[j]]
        tpt.set_camera(v[0:3], v[3:6], v[6], v[7], v[8])
        tpt.UpdateTest(t, first + j, w, h, flags)
        cams.append(tpt.GetSceneDesc()[2].copy())
        r0 = tpt.ray_counter_read()
        tpt.draw_device_moments(t, first + j, w, h, tile.data_ptr(), mo.data_ptr(), flags, albedo_ptr=out["albedo"][j].data_ptr(),
                                normal_depth_ptr=out["nd"][j].data_ptr())
        rays.append(tpt.ray_counter_read() - r0)  # (synchronises: the tile and the moments hold frame j)
        out["images"][j].copy_(tile)
        out["fmo"][j].copy_(mo)
    torch.cuda.synchronize()
    out.update(tile=tile, moments=mo, rays=rays, total=sum(rays), cams=np.concatenate(cams))
    return out


def assert_same_cameras(a, b):
    assert a["cams"].dtype == b["cams"].dtype and a["cams"].tobytes() == b["cams"].tobytes(), "the cameras differ from tptGetSceneDesc's"


def assert_same_as_sequence(tpt, w, h, times, views, first=0, flags=ANIMATED):
    a = draw_camera_clip(tpt, w, h, times, views, first, flags)
    tpt.set_camera(None)
    b = draw_camera_sequence(tpt, w, h, times, views, first, flags)
    assert_same(a, b, "the tptSetCamera + tptUpdate + tptDrawDeviceMoments sequence")
    assert_same_cameras(a, b)
    return a


def count_launches(tpt, w, h, times, views, flags):
    import torch
    n = len(times)
    tile, mo = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tpt.UpdateTest(times[0], 0, w, h, flags)
    tpt.kernel_timing_begin(2 * n)
    tpt.draw_device_camera_clip(times, views, 0, w, h, tile.data_ptr(), mo.data_ptr(), flags)
    ms, launches = tpt.kernel_timing_end()
    assert ms > 0.0
    return launches


# ---------------------------------------------------------------- 1. against the sequence
@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("flags", [ANIMATED, FLAG_ANIMATE], ids=["progressive", "each-frame-its-own"])
@pytest.mark.parametrize("n", [3, 33, 65])
def test_clip_equals_the_sequence(tpt_defaults, n, flags, first):
    """44 x 20: neither dimension a multiple of 8.  33 frames: two launches; 65: three, the staging's alternating halves reused"""
    w, h = 44, 20
    got = assert_same_as_sequence(tpt_defaults, w, h, irregular_times(n, seed=3), orbit_views(n), first, flags)
    assert np.array_equal(got["moments"][..., 3].cpu().numpy(), previous(w, h)[1][..., 3])  # (the moments' .w is nobody's to write)


# ---------------------------------------------------------------- 2. against the independent CPU statement
@pytest.mark.parametrize("flags", [ANIMATED, FLAG_ANIMATE], ids=["progressive", "each-frame-its-own"])
def test_three_frames_equal_the_checker(tpt_defaults, checker, oracle, flags):
    """32 x 16 x 4, three frames.  A kernel that traced every frame through one camera, or with one frame's seeds, must not pass: the
    test first asserts, with the checker alone, that frame 1 through frame 0's camera, and frame 1 with frame 0's seeds, each differ
    from frame 1's own normal / depth plane in at least a quarter of the pixels."""
    tpt = tpt_defaults
    w, h, n = 32, 16, 3
    times = irregular_times(n, seed=3)
    views = orbit_views(n)
    mats = oracle.default_scene()[1]
    spheres, _ = oracle.default_scene()
    bb, mo = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    want = []
    for j, t in enumerate(times):
        oracle.animate(spheres, t)
        cam = oracle_cam(oracle, views[j], w, h)
        r, _, _, alb, nd = checker.render(spheres, mats, cam, w, h, 4, j, flags, backbuffer=bb, moments=mo)
        want.append((r, bb.copy(), mo.copy(), alb, nd, cam))
        if j == 1:
            differ = lambda other: int((nd.view(np.int32) != other.view(np.int32)).any(axis=-1).sum())  # noqa: E731
            nd_cam0 = checker.render(spheres, mats, oracle_cam(oracle, views[0], w, h), w, h, 4, 1, flags)[4]
            nd_seed0 = checker.render(spheres, mats, cam, w, h, 4, 0, flags)[4]
            assert differ(nd_cam0) >= w * h // 4, ("frame 0's camera", differ(nd_cam0))
            assert differ(nd_seed0) >= w * h // 4, ("frame 0's seeds", differ(nd_seed0))
    zeros = (np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32))
    got = draw_camera_clip(tpt, w, h, times, views, 0, flags, prev=zeros)
    for j in range(n):
        r, image, moments, alb, nd, cam = want[j]
        assert got["rays"][j] == r, (j, got["rays"][j], r)
        assert got["cams"][j].tobytes() == cam.tobytes(), "frame %d: the camera differs from the oracle's" % j
        for k, ref in (("images", image), ("fmo", moments), ("albedo", alb), ("nd", nd)):
            assert got[k][j].cpu().numpy().tobytes() == ref.tobytes(), "frame %d: %s differs from the checker" % (j, k)
    assert got["tile"].cpu().numpy().tobytes() == bb.tobytes() and got["moments"].cpu().numpy().tobytes() == mo.tobytes()


# ---------------------------------------------------------------- 3. a clip in which nothing moves but the camera
@pytest.mark.parametrize("flags", [FLAG_PROGRESSIVE, 0], ids=["progressive", "each-frame-its-own"])
def test_static_clip_rides_the_same_kernel(tpt_defaults, flags):
    """no kFlagAnimate, 33 frames: the sequence's bytes from two trace launches, not 33, at two workgroups per CU"""
    tpt = tpt_defaults
    w, h, n = 44, 20, 33
    times, views = irregular_times(n, seed=4), orbit_views(n)
    assert_same_as_sequence(tpt, w, h, times, views, 2, flags)
    assert count_launches(tpt, w, h, times, views, flags) == 2
    assert tpt.launch_info()["blocks_per_cu"] == 2, tpt.launch_info()  # (the LDS of the single-frame twin)


def test_flat_scene_of_200_spheres(tpt_defaults):
    """a flat scene too large for the LDS beside two workgroups per CU (the kernel instantiated without the scene in LDS), animated and
    not: one launch per 32 frames, the sequence's bytes"""
    from test_gpu_animation import flat_scene
    from toypathtracer_amd.scenes import STRESS_CAMERA
    tpt = tpt_defaults
    tpt.set_scene(*flat_scene())
    w, h, n = 44, 20, 33
    c = STRESS_CAMERA
    views = orbit_views(n, height=c["look_from"][1], radius=c["look_from"][2], focus=c["focus_dist"])
    for flags in (ANIMATED, FLAG_PROGRESSIVE):
        times = irregular_times(n, seed=7)
        assert_same_as_sequence(tpt, w, h, times, views, 1, flags)
        assert count_launches(tpt, w, h, times, views, flags) == 2
    info = tpt.scene_info()
    assert info["spheres"] == 200 and info["groups"] == 0, info
    tpt.set_scene(None)


# ---------------------------------------------------------------- 4. the scenes that go frame by frame
@pytest.mark.parametrize("scene", ["eight-spheres", "256-spheres"])
def test_fallbacks_go_frame_by_frame(tpt_defaults, oracle, scene):
    """a scene the tptUpdate guard (Test.cpp:304) never moves, and a grouped one: the single-frame moments kernel with the camera set per
    frame, one launch per frame, the same bytes"""
    tpt = tpt_defaults
    if scene == "eight-spheres":
        s, m = oracle.default_scene()
        tpt.set_scene(s[:8].copy(), m[:8].copy())
    else:
        from toypathtracer_amd.scenes import stress_scene
        tpt.set_scene(*stress_scene(256, 16))
    w, h, n = 24, 16, 3
    times, views = irregular_times(n, seed=9), orbit_views(n)
    assert_same_as_sequence(tpt, w, h, times, views)
    assert tpt.scene_info()["spheres"] == (8 if scene == "eight-spheres" else 256)
    assert count_launches(tpt, w, h, times, views, ANIMATED) == n
    tpt.set_scene(None)


def test_one_trace_launch_per_32_frames(tpt_defaults):
    tpt = tpt_defaults
    for n in (1, 32, 33, 65):
        assert count_launches(tpt, 44, 20, [0.1 * k for k in range(n)], orbit_views(n), ANIMATED) == (n + 31) // 32, n
        assert tpt.launch_info()["blocks_per_cu"] == 2, tpt.launch_info()


# ---------------------------------------------------------------- 5. optional outputs, the cameras
@pytest.mark.parametrize("only", list(OUTPUTS) + ["none"])
def test_optional_outputs(tpt_defaults, only):
    """each of the five per-frame outputs alone, and none of them (outCameras NULL as well): what is asked for is what the call with
    every output gives, nothing else is written (draw_camera_clip checks the guard planes and that an output not asked for stays
    untouched)"""
    tpt = tpt_defaults
    w, h, n = 44, 20, 34
    times, views = irregular_times(n, seed=6), orbit_views(n)
    full = draw_camera_clip(tpt, w, h, times, views, 1)
    outputs = () if only == "none" else (only,)
    part = draw_camera_clip(tpt, w, h, times, views, 1, outputs=outputs, cameras=only != "none")
    assert_same(part, full, "the call with every output", outputs)
    if only != "none":
        assert_same_cameras(part, full)


@pytest.mark.parametrize("mitsuba", [False, True], ids=["default", "mitsuba-compare"])
def test_cameras_are_tptGetSceneDesc_s(tpt_defaults, oracle, mitsuba):
    """outCameras[j] is tptGetSceneDesc's camera after frame j's tptUpdate -- with the aperture forced to 0 in Mitsuba-compare mode --,
    and the planes are the sequence's there too"""
    tpt = tpt_defaults
    tpt.set_config(True, 0.9, mitsuba)
    w, h, n = 44, 20, 5
    times, views = irregular_times(n, seed=8), orbit_views(n)
    got = assert_same_as_sequence(tpt, w, h, times, views)
    assert all((c["lensRadius"] == 0.0) == mitsuba for c in got["cams"])
    for j in range(n):
        assert got["cams"][j].tobytes() == oracle_cam(oracle, views[j], w, h, mitsuba).tobytes(), j
    tpt.set_config()


# ---------------------------------------------------------------- 6. the context afterwards
def test_the_context_afterwards(tpt_defaults, oracle):
    """the camera of the last view and spheres 1 and 8 at the last time (tptGetSceneDesc); the next tptDrawDevice without a tptUpdate
    draws what it draws after the sequence; and a following tptDrawDeviceAnimationMoments, whose tptUpdate builds the camera from the
    set-up, renders through the last view"""
    import torch
    tpt = tpt_defaults
    w, h, n = 44, 20, 34
    times, views = irregular_times(n, seed=2), orbit_views(n)
    nxt = times[-1] + 0.3
    more = [nxt + 0.1 * k for k in range(3)]

    def after(out):
        s, _, cam, _ = tpt.GetSceneDesc()
        desc = (s.copy(), cam.copy())
        tpt.draw_device(nxt, n, w, h, out["tile"].data_ptr(), ANIMATED)
        tpt.synchronize()
        return desc, draw_clip(tpt, w, h, more, n + 1)

    a = draw_camera_clip(tpt, w, h, times, views)
    (sa, ca), clip_a = after(a)
    tpt.set_camera(None)
    b = draw_camera_sequence(tpt, w, h, times, views)
    (sb, cb), clip_b = after(b)
    torch.cuda.synchronize()
    assert ca.tobytes() == cb.tobytes() == a["cams"][-1].tobytes() == oracle_cam(oracle, views[-1], w, h).tobytes()
    want, _ = oracle.default_scene()
    oracle.animate(want, times[-1])
    assert sa.tobytes() == sb.tobytes()
    for i in (1, 8):
        assert [sa[i][k] for k in ("cx", "cy", "cz", "radius")] == [want[i][k] for k in ("cx", "cy", "cz", "radius")], i
    assert same(a["tile"], b["tile"]), "tptDrawDevice after the call differs from tptDrawDevice after the sequence"
    assert_same(clip_a, clip_b, "tptDrawDeviceAnimationMoments after the sequence")
    # (and it did render through the last view, not the default camera)
    tpt.set_camera(None)
    assert not same(clip_a["nd"][0], draw_clip(tpt, w, h, more, n + 1)["nd"][0])


# ---------------------------------------------------------------- 7. the chain the planes and the cameras are made for
def test_planes_and_cameras_feed_the_temporal_pass(tpt_defaults):
    """frames 1 and 2 of ONE call without the progressive flag, with the cameras it returned, through tptTemporalAccumulateDevice: the
    bytes the pass gives on the sequence's planes with tptGetSceneDesc's cameras"""
    import torch
    tpt = tpt_defaults
    w, h, n, flags = 44, 20, 3, FLAG_ANIMATE
    times, views = irregular_times(n, seed=5), orbit_views(n)
    zeros = (np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32))

    def chain(src):
        planes = lambda j: (src["images"][j], src["albedo"][j], src["nd"][j], src["fmo"][j])  # noqa: E731
        first = [torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in range(4)]
        second = [torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        tpt.temporal_accumulate_device(w, h, src["cams"][1], *[t.data_ptr() for t in planes(1)], *[t.data_ptr() for t in first])
        prev = (src["cams"][1], first[0].data_ptr(), first[1].data_ptr(), planes(1)[2].data_ptr(), first[2].data_ptr())
        tpt.temporal_accumulate_device(w, h, src["cams"][2], *[t.data_ptr() for t in planes(2)], *[t.data_ptr() for t in second], prev=prev)
        tpt.synchronize()
        return first + second

    a = chain(draw_camera_clip(tpt, w, h, times, views, 0, flags, prev=zeros))
    tpt.set_camera(None)
    b = chain(draw_camera_sequence(tpt, w, h, times, views, 0, flags, prev=zeros))
    assert all(same(x, y) for x, y in zip(a, b))
    assert all(bool(torch.isfinite(x[..., :3]).all()) for x in a)
