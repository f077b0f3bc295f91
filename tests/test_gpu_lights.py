"""The trace kernels across LIGHT COUNTS and LIGHT KINDS (tests/lights_lib.py), every image byte for byte and every frame's ray count
against the oracle.  The rest of the suite never has more than 8 lights, all small Lambert spheres far from every shading point; what
depends on the light list is exercised here:

  - the shadow loops of the path-queue and the lane-refill kernel with 0, 1, 15, 16, 17 and 46 lights -- metal, glass and the ground
    among them, so that a hit on a light skips itself --, the all-exact loop and the forward fold;
  - the LDS layout behind the light table, which the device code and the host's plan compute apart (a disagreement shows as wrong
    materials or path records: wrong pixels), at the 15 / 16 seam where the plan drops the LDS scene, with the scene forced in and out;
  - lights that enclose shading points, tiny and huge ones (the plain division of the light ray), coincident ones, one channel, a
    negative channel, a black albedo;
  - hundreds and thousands of lights: a flat scene read from global memory, one that keeps its place in LDS at one workgroup per CU, a
    grouped one, and the 4096-sphere scene up to the cap of include/tpt_hip.h -- 2864 lights fill a CU's LDS exactly, past that the
    lane-refill kernel takes the frame (its dynamic LDS above 48 KiB), 3073 are refused;
  - the other entry points' instantiations for a scene read from global memory, with lights that move.

tests/test_lights_plan.py holds the same plan on the CPU."""
import numpy as np
import pytest

import lights_lib
from adaptive_lib import AdaptiveChecker
from aov_lib import AovChecker
from common import describe_image_mismatch, oracle_frames
from moments_lib import MomentsChecker
from object_lib import ObjectChecker
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE, FOLD_FORWARD, FOLD_RECURSIVE, SEED_PER_PIXEL
from test_gpu_adaptive import draw_adaptive
from test_gpu_animation import draw_animation
from test_gpu_animation_moments import draw_clip
from test_gpu_aov import check as check_aov, draw_aov
from test_gpu_camera_clip import draw_camera_clip, oracle_cam, orbit_views
from test_gpu_keyframe_clip import draw_keyframe_clip, moved_centres, scene_of
from test_gpu_moments import check as check_moments, draw_moments
from test_gpu_parity import gpu_frames
from test_gpu_views import FOUR_VIEWS, check_against_oracle, draw_views

pytestmark = pytest.mark.gpu

ANIMATED = FLAG_PROGRESSIVE | FLAG_ANIMATE
DEFAULT, LANE_REFILL, ALL_EXACT = (0, 3, -1), (0, 1, -1), (1, 3, -1)
KERNELS = {"path_queues": (DEFAULT, FOLD_RECURSIVE), "lane_refill": (LANE_REFILL, FOLD_RECURSIVE), "all_exact": (ALL_EXACT, FOLD_RECURSIVE),
           "forward_fold": (DEFAULT, FOLD_FORWARD)}
CU_LDS = 160 * 1024  # gfx950: a CU's LDS

_wanted = {}


def stress_camera(oracle, w, h):
    from toypathtracer_amd.scenes import STRESS_CAMERA as c
    return c, oracle.camera(c["look_from"], c["look_at"], (0, 1, 0), c["vfov"], w / h, c["aperture"], c["focus_dist"])


def wanted(oracle, key, s, m, w, h, spp, frames, cam=None, fold=FOLD_RECURSIVE, light_sampling=True, first_frame=0, prev=None):
    """the oracle's frames of a scene (first_frame .. first_frame + frames - 1, blended into a copy of `prev`: a zeroed tile when None),
    rendered once per module and shared between the kernels that draw it -> (image, per-frame rays).  The caller's key tells two `prev`
    apart."""
    key = (key, w, h, spp, frames, fold, light_sampling, first_frame, prev is not None)
    if key not in _wanted:
        _, bo, pero = oracle_frames(oracle, w, h, spp, frames, spheres=s, mats=m, cam=cam, seed_mode=SEED_PER_PIXEL, fold_mode=fold,
                                    light_sampling=light_sampling, first=first_frame, bb=prev)
        assert np.isfinite(bo).all(), "the oracle's own image is not finite: the scene is no fair test (tests/lights_lib.py)"
        bo.setflags(write=False)
        _wanted[key] = (bo, pero)
    return _wanted[key]


def restore(tpt):
    tpt.set_scene(None)
    tpt.set_camera(None)
    tpt.set_samples_per_pixel(4)
    tpt.set_kernel_variant(0, 3, -1)
    tpt.set_fold_mode(FOLD_RECURSIVE)
    tpt.set_config(True, 0.9, False)


def draw(tpt, oracle, key, s, m, w, h, spp, frames, variant=DEFAULT, fold=FOLD_RECURSIVE, stress=False, light_sampling=True, camera=None,
         first_frame=0, prev=None):
    """the scene through DrawTest with this kernel, held against the oracle -> (launch_info(), scene_info(), per-frame rays); camera: the
    keyword arguments of tpt.set_camera (stress: STRESS_CAMERA), None for the default camera; the frames are first_frame ..
    first_frame + frames - 1, blended into a copy of the tile `prev` (a zeroed one when None)"""
    cam = None
    try:
        tpt.set_scene(s, m)
        if stress:
            c, cam = stress_camera(oracle, w, h)
            tpt.set_camera(**c)
        elif camera is not None:
            cam = oracle.camera(camera["look_from"], camera["look_at"], (0, 1, 0), camera["vfov"], w / h, camera["aperture"], camera["focus_dist"])
            tpt.set_camera(**camera)
        tpt.set_samples_per_pixel(spp)
        tpt.set_kernel_variant(*variant)
        tpt.set_fold_mode(fold)
        tpt.set_config(light_sampling, 0.9, False)
        _, bb, per = gpu_frames(tpt, w, h, frames, bb=None if prev is None else np.ascontiguousarray(prev, np.float32).copy(), first=first_frame)
        info, scene = tpt.launch_info(), tpt.scene_info()
    finally:
        restore(tpt)
    bo, pero = wanted(oracle, key, s, m, w, h, spp, frames, cam, fold, light_sampling, first_frame, prev)
    assert per == pero, (key, variant, per, pero)
    assert bb.tobytes() == bo.tobytes(), describe_image_mismatch(bb, bo)
    return info, scene, per


# ---------------------------------------------------------------- 1. light counts on the built-in scene
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("k", lights_lib.LIGHT_COUNTS)
def test_light_counts(tpt_defaults, oracle, k, kernel):
    variant, fold = KERNELS[kernel]
    s, m = lights_lib.default_with_lights(k, seed=k + 1)
    info, _, per = draw(tpt_defaults, oracle, ("count", k), s, m, 96, 54, 2, 2, variant, fold)
    assert info["blocks_per_cu"] >= 1
    if kernel == "path_queues":
        assert info["blocks_per_cu"] == 2


def test_the_16th_light_costs_the_lds_scene_not_the_second_workgroup(tpt_defaults, oracle):
    """two workgroups per CU are worth more than the scene in LDS.  The <false> instantiation of the default kernel (no
    LDS scene, no matrix-core filter) runs from 16 lights on."""
    infos = {}
    for k in (15, 16):
        s, m = lights_lib.default_with_lights(k, seed=k + 1)
        infos[k], _, _ = draw(tpt_defaults, oracle, ("count", k), s, m, 96, 54, 2, 2)
    assert infos[15]["blocks_per_cu"] == 2 and infos[16]["blocks_per_cu"] == 2, infos
    assert infos[16]["lds_bytes"] < infos[15]["lds_bytes"], infos


@pytest.mark.parametrize("lds_scene", [1, 0], ids=["lds_scene_forced", "lds_scene_off"])
@pytest.mark.parametrize("k", [15, 16])
def test_the_seam_with_the_lds_scene_forced_in_and_out(tpt_defaults, oracle, k, lds_scene):
    s, m = lights_lib.default_with_lights(k, seed=k + 1)
    auto, _, _ = draw(tpt_defaults, oracle, ("count", k), s, m, 96, 54, 2, 2)
    info, _, _ = draw(tpt_defaults, oracle, ("count", k), s, m, 96, 54, 2, 2, (0, 3, lds_scene))
    # (the plan's own choice is one of the two: the scene in LDS up to 15 lights, out of it from 16 on)
    assert (info["lds_bytes"] == auto["lds_bytes"]) == (lds_scene == (1 if k == 15 else 0)), (auto, info)
    assert info["blocks_per_cu"] == (1 if (lds_scene, k) == (1, 16) else 2), info


def test_46_lights_without_light_sampling(tpt_defaults, oracle):
    """every sphere a light and the light loop compiled out (Test.cpp:95): the ray count is the one without shadow rays"""
    s, m = lights_lib.default_with_lights(46, seed=47)
    _, _, per = draw(tpt_defaults, oracle, ("count", 46), s, m, 96, 54, 2, 2, light_sampling=False)
    _, with_shadow_rays = wanted(oracle, ("count", 46), s, m, 96, 54, 2, 2)
    assert all(a < b for a, b in zip(per, with_shadow_rays)), (per, with_shadow_rays)


# ---------------------------------------------------------------- 2. light kinds
@pytest.mark.parametrize("kernel", ["path_queues", "lane_refill"])
@pytest.mark.parametrize("kind", lights_lib.LIGHT_KINDS)
def test_light_kinds(tpt_defaults, oracle, kind, kernel):
    s, m = lights_lib.light_kind(kind)
    assert lights_lib.r2_div_safe(s, m) == (kind not in ("tiny", "huge"))  # (those two take the plain division of the light ray)
    draw(tpt_defaults, oracle, ("kind", kind), s, m, 96, 54, 2, 2, KERNELS[kernel][0])


# ---------------------------------------------------------------- 3. many lights
def test_150_lights_on_a_flat_scene_read_from_global_memory(tpt_defaults, oracle):
    s, m = lights_lib.stress_with_lights(200, 16, 150)
    info, scene, _ = draw(tpt_defaults, oracle, "flat200", s, m, 64, 32, 1, 2, stress=True)
    forced, _, _ = draw(tpt_defaults, oracle, "flat200", s, m, 64, 32, 1, 2, (0, 3, 1), stress=True)
    assert scene["groups"] == 0, scene
    assert info["blocks_per_cu"] == 2 and info["lds_bytes"] < forced["lds_bytes"], (info, forced)  # (the scene left LDS for the second workgroup)


def test_350_lights_beside_the_groups_bounds(tpt_defaults, oracle):
    """400 spheres are a grouped scene (no LDS scene), whose groups' bounds sit in LDS for the second filter level -- unless the launch
    would lose its second workgroup per CU with them there: chooseKernel's "many lights beside them".  100 lights leave both; 350 lights
    cost the second workgroup, and the bounds are read from global memory."""
    few, scene_few, _ = draw(tpt_defaults, oracle, "grouped400/100", *lights_lib.stress_with_lights(400, 20, 100), 64, 32, 1, 2, stress=True)
    many, scene, _ = draw(tpt_defaults, oracle, "grouped400/350", *lights_lib.stress_with_lights(400, 20, 350), 64, 32, 1, 2, stress=True)
    assert scene["groups"] > 0 and scene == scene_few, (scene, scene_few)
    assert few["blocks_per_cu"] == 2 and many["blocks_per_cu"] == 1, (few, many)
    assert 0 < many["lds_bytes"] - few["lds_bytes"] < 250 * 32, (few, many)  # (250 lights more, and the bounds gone)


def test_300_lights_on_a_grouped_scene(tpt_defaults, oracle):
    s, m = lights_lib.stress_with_lights(1000, 20, 300)
    info, scene, _ = draw(tpt_defaults, oracle, "grouped1000", s, m, 64, 32, 1, 2, stress=True)
    assert scene["groups"] > 0, scene
    assert info["blocks_per_cu"] >= 1


@pytest.mark.parametrize("kernel", ["path_queues", "lane_refill"])
def test_1024_lights_on_4096_spheres(tpt_defaults, oracle, kernel):
    s, m = lights_lib.stress_with_lights(4096, 64, 1024)
    info, scene, _ = draw(tpt_defaults, oracle, "stress1024", s, m, 32, 16, 1, 1, KERNELS[kernel][0], stress=True)
    assert scene["groups"] > 0 and info["blocks_per_cu"] >= 1, (scene, info)


def test_2864_lights_fill_a_cu_and_still_count_as_one_workgroup(tpt_defaults, oracle):
    s, m = lights_lib.stress_with_lights(4096, 64, 2864)
    info, _, _ = draw(tpt_defaults, oracle, "stress2864", s, m, 16, 8, 1, 1, stress=True)
    assert info["blocks_per_cu"] >= 1, info
    assert info["lds_bytes"] <= CU_LDS and info["grid_blocks"] >= 1, info


@pytest.mark.parametrize("kernel", ["path_queues", "lane_refill"])
def test_3072_lights_the_stated_cap(tpt_defaults, oracle, kernel):
    """the default configuration plans this frame on the lane-refill kernel (the path-queue kernel's LDS holds fewer lights beside this
    scene), as the host that asks for that kernel gets it: more than 48 KiB of dynamic LDS either way"""
    s, m = lights_lib.stress_with_lights(4096, 64, 3072)
    info, _, _ = draw(tpt_defaults, oracle, "stress3072", s, m, 16, 8, 1, 1, KERNELS[kernel][0], stress=True)
    assert info["blocks_per_cu"] >= 1 and 48 * 1024 < info["lds_bytes"] <= CU_LDS, info


def test_3073_lights_are_refused(tpt_defaults, oracle):
    import torch
    tpt = tpt_defaults
    w, h = 16, 8
    s, m = lights_lib.stress_with_lights(4096, 64, 3073)
    before = np.random.default_rng(5).random((h, w, 4), dtype=np.float32)
    tile = torch.from_numpy(before).cuda()
    try:
        tpt.set_scene(s, m)
        tpt.set_samples_per_pixel(1)
        tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
        with pytest.raises(tpt.TptError):
            tpt.draw_device(0.0, 0, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
        message = tpt.load_library().tptGetLastError().decode()
        assert "too many emissive spheres" in message and "3072 at most" in message, message
        tpt.synchronize()
        assert tile.cpu().numpy().tobytes() == before.tobytes(), "a refused draw wrote the tile"
    finally:
        restore(tpt)
    # the next draw, of the built-in scene, as if nothing had happened
    _, bb, per = gpu_frames(tpt, 96, 54, 2)
    _, bo, pero = oracle_frames(oracle, 96, 54, 4, 2, seed_mode=SEED_PER_PIXEL)
    assert per == pero and bb.tobytes() == bo.tobytes()


# ---------------------------------------------------------------- 4. the other entry points: 20 lights, the scene read from global memory
W, H, SPP, N = 66, 35, 2, 3


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """the existing modules' CPU statements of the planes, built on first use and once"""
    built = {}

    def get(cls):
        if cls not in built:
            built[cls] = cls(tmp_path_factory.mktemp(cls.__name__))
        return built[cls]
    return get


@pytest.fixture()
def twenty(tpt_defaults):
    """default_with_lights(20): spheres 1..20 are lights -- both spheres kFlagAnimate moves among them -- and the launches take the
    instantiations without the LDS scene"""
    tpt = tpt_defaults
    s, m = lights_lib.default_with_lights(20, seed=21)
    tpt.set_scene(s, m)
    tpt.set_samples_per_pixel(SPP)
    try:
        yield tpt, s, m
    finally:
        restore(tpt)


def two_workgroups_no_lds_scene(tpt):
    info = tpt.launch_info()
    assert info["blocks_per_cu"] == 2, info
    return info


def test_views(twenty, oracle):
    tpt, s, m = twenty
    views = FOUR_VIEWS[:2]
    tiles, per = draw_views(tpt, W, H, views, range(N))
    two_workgroups_no_lds_scene(tpt)
    check_against_oracle(oracle, tiles, per, views, W, H, SPP, N, spheres=s, mats=m)


def test_animation(twenty, oracle):
    tpt, s, m = twenty
    times = [0.4 * j for j in range(N)]
    tile, images, per = draw_animation(tpt, W, H, times)
    two_workgroups_no_lds_scene(tpt)
    spheres, cam, bo, got = s.copy(), oracle.default_camera(W, H), np.zeros((H, W, 4), np.float32), images.cpu().numpy()
    for f, t in enumerate(times):
        oracle.animate(spheres, t)
        r, _ = oracle.render(spheres, m, cam, W, H, SPP, f, ANIMATED, backbuffer=bo, seed_mode=SEED_PER_PIXEL)
        assert per[f] == r, (f, per[f], r)
        assert got[f].tobytes() == bo.tobytes(), "frame %d differs from the oracle" % f
    assert tile.cpu().numpy().tobytes() == bo.tobytes()


def test_aov(twenty, oracle, checkers):
    tpt, s, m = twenty
    got = draw_aov(tpt, W, H, range(N))
    two_workgroups_no_lds_scene(tpt)
    check_aov(checkers(AovChecker), oracle, got, W, H, SPP, N, spheres=s, mats=m)


def test_moments(twenty, oracle, checkers):
    tpt, s, m = twenty
    got = draw_moments(tpt, W, H, range(N))
    two_workgroups_no_lds_scene(tpt)
    check_moments(checkers(MomentsChecker), oracle, got, W, H, SPP, N, spheres=s, mats=m)


def test_adaptive(twenty, oracle, checkers):
    tpt, s, m = twenty
    counts = np.random.default_rng(3).choice(np.int32([0, 1, 2, 3, 5]), size=(H, W)).astype(np.int32)
    got = draw_adaptive(tpt, W, H, range(N), counts)
    two_workgroups_no_lds_scene(tpt)
    per, bb, mo, alb, nd = checkers(AdaptiveChecker).frames(oracle, W, H, counts, N, spheres=s, mats=m)
    assert got[4] == per
    for name, g, want in zip(("tile", "moments", "albedo", "normal / depth"), got[:4], (bb, mo, alb, nd)):
        assert g.tobytes() == want.tobytes(), "the %s differs from the checker" % name


def clip_against_the_checker(checker, got, frames):
    """frames: (spheres, camera) per frame -> every per-frame output, the tile and the moments against the moments checker's chain"""
    bb, mo = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    for j, (spheres, mats, cam, flags) in enumerate(frames):
        r, _, _, alb, nd = checker.render(spheres, mats, cam, W, H, SPP, j, flags, backbuffer=bb, moments=mo)
        assert got["rays"][j] == r, (j, got["rays"][j], r)
        for k, ref in (("images", bb), ("fmo", mo), ("albedo", alb), ("nd", nd)):
            assert got[k][j].cpu().numpy().tobytes() == ref.tobytes(), "frame %d: %s differs from the checker" % (j, k)
    assert got["tile"].cpu().numpy().tobytes() == bb.tobytes() and got["moments"].cpu().numpy().tobytes() == mo.tobytes()


ZEROS = (np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32))


def animated_frames(oracle, s, m, times, cams):
    spheres, out = s.copy(), []
    for t, cam in zip(times, cams):
        oracle.animate(spheres, t)
        out.append((spheres.copy(), m, cam, ANIMATED))
    return out


def test_animation_moments(twenty, oracle, checkers):
    tpt, s, m = twenty
    times = [0.4 * j for j in range(N)]
    got = draw_clip(tpt, W, H, times, 0, ANIMATED, prev=ZEROS)
    two_workgroups_no_lds_scene(tpt)
    clip_against_the_checker(checkers(MomentsChecker), got, animated_frames(oracle, s, m, times, [oracle.default_camera(W, H)] * N))


def test_camera_clip(twenty, oracle, checkers):
    tpt, s, m = twenty
    times, views = [0.4 * j for j in range(N)], orbit_views(N)
    got = draw_camera_clip(tpt, W, H, times, views, 0, ANIMATED, prev=ZEROS)
    two_workgroups_no_lds_scene(tpt)
    cams = [oracle_cam(oracle, views[j], W, H) for j in range(N)]
    for j in range(N):
        assert got["cams"][j].tobytes() == cams[j].tobytes(), "frame %d: the camera differs from the oracle's" % j
    clip_against_the_checker(checkers(MomentsChecker), got, animated_frames(oracle, s, m, times, cams))


def test_keyframe_clip(twenty, oracle, checkers):
    """the caller moves four spheres, three of them lights (a Lambert, a metal and the Lambert sphere 8) and one not"""
    tpt, s, m = twenty
    ids = [8, 30, 1, 5]
    assert [i in lights_lib.light_ids(m) for i in ids] == [True, False, True, True]
    views, centres = orbit_views(N), moved_centres(s, ids, N, seed=2)
    got = draw_keyframe_clip(tpt, W, H, (s, m), views, ids, centres, 0, FLAG_PROGRESSIVE, prev=ZEROS)
    two_workgroups_no_lds_scene(tpt)
    cams = [oracle_cam(oracle, views[j], W, H) for j in range(N)]
    clip_against_the_checker(checkers(MomentsChecker), got, [(scene_of(s, ids, centres, j), m, cams[j], FLAG_PROGRESSIVE) for j in range(N)])
    objects, object_checker = got["objects"].cpu().numpy(), checkers(ObjectChecker)
    for j in range(N):
        assert got["cams"][j].tobytes() == cams[j].tobytes(), "frame %d: the camera differs from the oracle's" % j
        want = object_checker.plane(scene_of(s, ids, centres, j), got["cams"][j:j + 1], W, H)
        assert objects[j].tobytes() == want[0].tobytes(), "frame %d: the object plane differs from the oracle's HitSpheres" % j
