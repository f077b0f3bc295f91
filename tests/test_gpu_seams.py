"""The trace kernels AT THE LIMITS OF THEIR PACKED FIELDS (tests/seams_lib.py), every image byte for byte and every ray count against the
oracle.  The path-queue kernel carries a path's sample index, depth and hit id, and a pixel's column, row and frame of the batch, as
integers in float-typed LDS words; the host sends a frame to the lane-refill kernel, or refuses the call, where a field would overflow.
The rest of the suite stays far inside every field (16 samples, 4096 spheres, frame numbers below 300, 3840 columns).  Held here:

  - 17 ... 2047 samples per pixel on the path-queue kernel (the 11-bit sample field, the decision that a sample is its pixel's last),
    2048, 2049 and 65536 on the kernel the host takes instead, with the same bytes; 2047 through the planes' sums; sample counts of 2046,
    2047, 2048 and 5000 side by side in one adaptive frame;
  - sphere ids up to 65533 through the record word -- first hits, bounce rays off glass and metal, the planes' first-hit sums and the
    object plane -- in a grouped scene of 65534 spheres, and the 65535th sphere on the lane-refill kernel; HitSpheres itself on both;
  - frames of 65535 columns and of 65535 rows, whose rows 32640..32767 and 65408..65534 make NaN bit patterns of the pixel word, and
    65536 on the other kernel; batches of 31, 32 and 33 frames of 8192 rows and of 8192 columns on the frame-pools kernel, a clip of 32
    such frames with its planes: slot 31's rows 7168..8191 are the batched word's NaN patterns;
  - frame numbers 2^24 - 1 ... 2^31 - 2 in the seeds and in the blend, single and three per launch;
  - that the kernel which ran at a limit is another one than past it (tptGetLaunchInfo).

tests/test_seams.py proves on the CPU that every case is what it claims and holds the host's routing on the emulated runtime."""
import numpy as np
import pytest

import seams_lib as lib
from adaptive_lib import AdaptiveChecker
from aov_lib import AovChecker
from common import describe_image_mismatch, grazing_rays
from moments_lib import MomentsChecker
from object_lib import ObjectChecker
from oracle_lib import FLAG_PROGRESSIVE
from test_gpu_adaptive import draw_adaptive
from test_gpu_aov import check as check_aov, draw_aov
from test_gpu_batch_moments import NAMES, call as call_batch_moments
from test_gpu_camera_clip import draw_camera_clip
from test_gpu_lights import draw, restore
from test_gpu_moments import check as check_moments, draw_moments
from test_gpu_objects import object_planes
from test_gpu_parity import _batched, gpu_frames
from test_gpu_scene_kinds import VARIANTS, oracle_hits, rays_that_hit
from test_seams import checkers, first_hit_plane, previous, start_planes, wanted  # noqa: F401  (checkers: a module fixture)

pytestmark = pytest.mark.gpu

MAIN = ("path_queues", "lane_refill")
OTHERS = ("all_exact", "forward_fold", "valu_filter", "one_thread_per_pixel")
AT_A_SEAM = tuple(n for pair in lib.SEAM_PAIRS for n in pair)
SINGLE = tuple(n for n in lib.CASES if lib.ENTRY[n] == "draw" and lib.FAMILY_OF[n] != "sphere_ids")


def draw_case(tpt, oracle, name, kernel):
    """a case of single frames through DrawTest on this kernel, against the oracle -> launch_info()"""
    variant, fold = VARIANTS[kernel]
    s, m, camera, w, h, spp, first, frames = lib.build(name)
    prev = previous(name) if lib.FAMILY_OF[name] == "frame_numbers" else None
    if lib.FLAGS[name] == FLAG_PROGRESSIVE:
        info, _, _ = draw(tpt, oracle, ("seam", name), s, m, w, h, spp, frames, variant, fold, camera=camera, first_frame=first, prev=prev)
        return info
    # without the progressive flag: the tile is the frame alone
    assert camera is None and fold == VARIANTS["path_queues"][1]
    try:
        tpt.set_samples_per_pixel(spp)
        tpt.set_kernel_variant(*variant)
        _, bb, per = gpu_frames(tpt, w, h, frames, flags=lib.FLAGS[name], bb=prev.copy(), first=first)
        info = tpt.launch_info()
    finally:
        restore(tpt)
    want = wanted(oracle, name)
    assert per == want["rays"], (name, kernel, per, want["rays"])
    assert bb.tobytes() == want["tile"].tobytes(), describe_image_mismatch(bb, want["tile"])
    return info


def kernel_of(info):
    """what tells the two kernels apart in tptGetLaunchInfo: the LDS of a workgroup and the workgroups a CU holds"""
    return info["lds_bytes"], info["blocks_per_cu"]


# ---------------------------------------------------------------- 1. samples, extents, frame numbers: single frames
@pytest.mark.parametrize("kernel", MAIN)
@pytest.mark.parametrize("name", SINGLE)
def test_single_frames(tpt_defaults, oracle, name, kernel):
    info = draw_case(tpt_defaults, oracle, name, kernel)
    assert info["blocks_per_cu"] >= 1, info
    if kernel == "path_queues" and lib.path_queue_side(name):
        assert info["blocks_per_cu"] == 2, info  # (the built-in scene on the path-queue kernel: DESIGN 3.2)


@pytest.mark.parametrize("kernel", OTHERS)
@pytest.mark.parametrize("name", AT_A_SEAM)
def test_the_seam_values_on_the_other_variants(tpt_defaults, oracle, name, kernel):
    draw_case(tpt_defaults, oracle, name, kernel)


@pytest.mark.parametrize("at,past", lib.SEAM_PAIRS + (("spheres_65534", "spheres_65535"),), ids=lambda n: n)
def test_another_kernel_runs_past_the_limit(tpt_defaults, oracle, at, past):
    """a context that asks for the path-queue kernel gets it at the limit and the lane-refill kernel one past it -- the launch the
    context that asks for the lane-refill kernel makes of the same frame"""
    tpt = tpt_defaults
    assert lib.path_queue_side(at) and not lib.path_queue_side(past)
    run = draw_scene if lib.FAMILY_OF[at] == "sphere_ids" else draw_case
    at_limit, past_limit = kernel_of(run(tpt, oracle, at, "path_queues")), kernel_of(run(tpt, oracle, past, "path_queues"))
    refill_at, refill_past = kernel_of(run(tpt, oracle, at, "lane_refill")), kernel_of(run(tpt, oracle, past, "lane_refill"))
    assert at_limit != past_limit, (at_limit, past_limit)
    assert at_limit != refill_at and past_limit == refill_past, (at_limit, refill_at, past_limit, refill_past)


# ---------------------------------------------------------------- 2. sphere ids
def draw_scene(tpt, oracle, name, kernel):
    variant, fold = VARIANTS[kernel]
    s, m, camera, w, h, spp, first, frames = lib.build(name)
    info, scene, _ = draw(tpt, oracle, ("seam", name), s, m, w, h, spp, frames, variant, fold, camera=camera)
    assert scene["spheres"] == len(s) and scene["groups"] > 0, scene
    assert info["blocks_per_cu"] >= 1, info
    return info


@pytest.mark.parametrize("kernel", MAIN)
@pytest.mark.parametrize("name", lib.FAMILIES["sphere_ids"])
def test_many_sphere_scenes(tpt_defaults, oracle, name, kernel):
    draw_scene(tpt_defaults, oracle, name, kernel)


@pytest.fixture()
def many(tpt_defaults):
    """the 65534-sphere scene set, at its case's samples per pixel"""
    tpt = tpt_defaults
    s, m, camera, w, h, spp, _, _ = lib.build("spheres_65534")
    assert camera is None
    tpt.set_scene(s, m)
    tpt.set_samples_per_pixel(spp)
    try:
        yield tpt, s, m, w, h, spp
    finally:
        restore(tpt)


def test_many_spheres_aov(many, oracle, checkers):  # noqa: F811
    tpt, s, m, w, h, spp = many
    alb, nd = check_aov(checkers(AovChecker), oracle, draw_aov(tpt, w, h, [0]), w, h, spp, 1, spheres=s, mats=m)
    assert np.isfinite(alb).all() and np.isfinite(nd).all()


def test_many_spheres_moments(many, oracle, checkers):  # noqa: F811
    tpt, s, m, w, h, spp = many
    check_moments(checkers(MomentsChecker), oracle, draw_moments(tpt, w, h, [0]), w, h, spp, 1, spheres=s, mats=m)


def test_many_spheres_object_plane(many, oracle, checkers):  # noqa: F811
    tpt, s, m, w, h, _ = many
    tpt.UpdateTest(0.0, 0, w, h, 0)
    cam = tpt.GetSceneDesc()[2]
    got = object_planes(tpt, w, h)
    tpt.synchronize()
    got = got.cpu().numpy()
    assert got.tobytes() == checkers(ObjectChecker).plane(s, cam, w, h).tobytes()
    assert got[0].tobytes() == first_hit_plane(oracle, checkers, "spheres_65534").tobytes()
    assert set(lib.planted(len(s))) <= set(np.unique(got).tolist()), "a planted index is missing from the object plane"


@pytest.mark.parametrize("name", lib.FAMILIES["sphere_ids"])
def test_hit_spheres_vs_oracle_on_the_planted_spheres(tpt_hooks, oracle, name):
    """rays that graze the planted spheres and the camera's own, through both traversals: ids equal, t bit-equal"""
    from object_lib import centre_rays
    tpt = tpt_hooks
    s, m, camera, w, h, _, _, _ = lib.build(name)
    planted = sorted(lib.planted(len(s)))
    o, d = centre_rays(lib.oracle_camera(oracle, camera, w, h), w, h)
    cam_rays = np.concatenate([np.broadcast_to(o, (h * w, 3)), np.stack([c.reshape(-1) for c in d], 1)], 1).astype(np.float32)

    def make(seed):
        return np.ascontiguousarray(np.concatenate([grazing_rays(s[planted], 1000, seed=seed), cam_rays], 0))
    rays, want_id, want_t = rays_that_hit(make, lambda r: oracle_hits(oracle, s, r))
    assert set(planted) <= set(want_id.tolist())
    try:
        tpt.set_scene(s, m)
        tpt.UpdateTest(0.0, 0, 64, 64, 2)
        assert tpt.scene_info()["groups"] > 0
        for hs in (0, 1):
            ids, ts = tpt.test_hit_spheres(rays, hs)
            assert np.array_equal(ids, want_id), (hs, int((ids != want_id).sum()))
            assert np.array_equal(ts.view(np.uint32), want_t.view(np.uint32)), hs
    finally:
        tpt.set_scene(None)


# ---------------------------------------------------------------- 3. 2047 samples through the planes' sums
W, H = 8, 8


@pytest.fixture()
def spp_2047(tpt_defaults):
    tpt_defaults.set_samples_per_pixel(lib.MAX_SPP)
    try:
        yield tpt_defaults
    finally:
        restore(tpt_defaults)


def test_2047_samples_aov(spp_2047, oracle, checkers):  # noqa: F811
    alb, _ = check_aov(checkers(AovChecker), oracle, draw_aov(spp_2047, W, H, [0]), W, H, lib.MAX_SPP, 1)
    cov = alb[..., 3].astype(np.float64) * lib.MAX_SPP
    assert np.abs(cov - np.round(cov)).max() < 1e-3 and ((cov > 0.5) & (cov < lib.MAX_SPP - 0.5)).any()  # (counts of hits, some pixels on an edge)


def test_2047_samples_moments(spp_2047, oracle, checkers):  # noqa: F811
    check_moments(checkers(MomentsChecker), oracle, draw_moments(spp_2047, W, H, [0]), W, H, lib.MAX_SPP, 1)


def test_adaptive_counts_around_the_clamp(tpt_defaults, oracle, checkers):  # noqa: F811
    """2046, 2047, 2048 and 5000 samples asked for side by side: the last two are clamped to 2047 where a lane claims the pixel"""
    counts = np.tile(np.int32([2046, 2047, 2048, 5000, 1, 2047, 0, 2048]), (H, 1))
    got = draw_adaptive(tpt_defaults, W, H, [0], counts)
    per, bb, mo, alb, nd = checkers(AdaptiveChecker).frames(oracle, W, H, counts, 1)
    assert got[4] == per
    for what, g, want in zip(("tile", "moments", "albedo", "normal / depth"), got[:4], (bb, mo, alb, nd)):
        assert g.tobytes() == want.tobytes(), "the %s differs from the checker" % what
    assert (got[1][..., 3] == np.clip(counts, 0, lib.MAX_SPP)).all()


# ---------------------------------------------------------------- 4. batched extents and frame numbers
def batched_case(tpt, oracle, name, sizes=None, first=None, prev=None):
    """tptDrawDeviceBatch once per entry of `sizes` (the whole case in one call when None) -> (rays, tile)"""
    _, _, camera, w, h, spp, first0, frames = lib.build(name)
    try:
        if camera is not None:
            tpt.set_camera(**camera)
        return _batched(tpt, w, h, sizes or [frames], lib.FLAGS[name], spp, first0 if first is None else first,
                        previous(name) if prev is None else prev)
    finally:
        restore(tpt)


@pytest.mark.parametrize("name", [n for n in lib.CASES if lib.ENTRY[n] == "batch"])
def test_batches(tpt_defaults, oracle, name):
    rays, tile = batched_case(tpt_defaults, oracle, name)
    want = wanted(oracle, name)
    assert rays == sum(want["rays"]), (rays, sum(want["rays"]))
    assert tile.tobytes() == want["tile"].tobytes(), describe_image_mismatch(tile, want["tile"])
    assert tpt_defaults.launch_info()["blocks_per_cu"] >= 1


@pytest.mark.parametrize("shape", ["2x8192", "8192x2"])
def test_the_33_frames_launch_by_launch(tpt_defaults, oracle, shape):
    """the launch of 32 and the launch of 1 the call of 33 frames makes, each held on its own: the tile and the rays after 32 frames are
    the 32-frame case's, the 33rd frame continues from there"""
    name = "batch_%s_x33" % shape
    after32, after33 = wanted(oracle, "batch_%s_x32" % shape), wanted(oracle, name)
    rays, tile = batched_case(tpt_defaults, oracle, name, sizes=[32])
    assert rays == sum(after32["rays"]) == sum(after33["rays"][:32])
    assert tile.tobytes() == after32["tile"].tobytes(), describe_image_mismatch(tile, after32["tile"])
    rays, tile = batched_case(tpt_defaults, oracle, name, sizes=[1], first=32, prev=tile)
    assert rays == after33["rays"][32]
    assert tile.tobytes() == after33["tile"].tobytes(), describe_image_mismatch(tile, after33["tile"])


@pytest.mark.parametrize("name", [n for n in lib.CASES if lib.ENTRY[n] == "batch_moments"])
def test_batch_moments(tpt_defaults, oracle, checkers, name):  # noqa: F811
    tpt = tpt_defaults
    _, _, camera, w, h, spp, first, frames = lib.build(name)
    assert camera is None
    want = wanted(oracle, name, checkers)
    try:
        tpt.set_samples_per_pixel(spp)
        got, rays = call_batch_moments(tpt, w, h, first, [frames], lib.FLAGS[name], list(start_planes(name)))
    finally:
        restore(tpt)
    assert rays == sum(want["rays"])
    for what, g, key in zip(NAMES, got, ("tile", "moments", "albedo", "nd")):
        assert g.tobytes() == want[key].tobytes(), "%s differs from the CPU statement" % what


def test_camera_clip_of_32_tall_frames(tpt_defaults, oracle, checkers):  # noqa: F811
    """the clip kernel (a batched launch without frame pools) with its planes: slot 31's rows 7168..8191"""
    tpt = tpt_defaults
    name = "clip_2x8192_x32"
    _, _, camera, w, h, spp, first, frames = lib.build(name)
    c = camera
    views = np.float32([list(c["look_from"]) + list(c["look_at"]) + [c["vfov"], c["aperture"], c["focus_dist"]]] * frames)
    want = wanted(oracle, name, checkers)
    start = start_planes(name)
    try:
        tpt.set_samples_per_pixel(spp)
        got = draw_camera_clip(tpt, w, h, [0.0] * frames, views, first, lib.FLAGS[name], prev=(start[0], start[1]))
        info = tpt.launch_info()
    finally:
        restore(tpt)
    assert got["rays"] == want["rays"]
    cam = lib.oracle_camera(oracle, camera, w, h)
    for j in range(frames):
        assert got["cams"][j].tobytes() == cam.tobytes(), "frame %d: the camera differs from the oracle's" % j
        for k, ref in (("images", "images"), ("fmo", "fmo"), ("albedo", "f_albedo"), ("nd", "f_nd")):
            assert got[k][j].cpu().numpy().tobytes() == want[ref][j].tobytes(), "frame %d: %s differs from the checker" % (j, k)
    assert got["tile"].cpu().numpy().tobytes() == want["tile"].tobytes() and got["moments"].cpu().numpy().tobytes() == want["moments"].tobytes()
    assert info["blocks_per_cu"] >= 1, info
