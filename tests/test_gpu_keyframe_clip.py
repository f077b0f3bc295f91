"""tptDrawDeviceKeyframeClip on the GPU: the frames of a clip whose spheres the CALLER moves, a camera per frame, each with its denoiser
planes and its object plane, up to 32 per launch.  Every frame's image, albedo, normal / depth, moments plane, object plane, ray count
and Camera record, the final tile and the final moments are held byte for byte (no tolerance anywhere) against the tptSetScene +
tptSetCamera + tptUpdate + tptDrawDeviceMoments sequence the call replaces and against the CPU statement of the trace
(tests/moments_checker.c) over each frame's spheres; then against tptDrawDeviceCameraClip where the two calls say the same, the launch
counts and the calls that go frame by frame, the optional outputs, the object planes against the oracle's HitSpheres, the context
afterwards, the object-following temporal pass on the call's planes, and refusals."""
import ctypes as C

import numpy as np
import pytest

from moments_lib import MomentsChecker
from object_lib import ObjectChecker
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE
from test_gpu_animation import flat_scene, irregular_times
from test_gpu_animation_moments import GUARD, OUTPUTS, assert_same, guarded, guards_intact, previous, same
from test_gpu_camera_clip import draw_camera_clip, oracle_cam, orbit_views

pytestmark = pytest.mark.gpu

ALL = OUTPUTS + ("objects",)
LAMBERT, METAL, DIELECTRIC = 0, 1, 2  # (Material::Type, Test.cpp)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return MomentsChecker(tmp_path_factory.mktemp("moments_checker"))


@pytest.fixture(scope="module")
def object_checker(tmp_path_factory):
    return ObjectChecker(tmp_path_factory.mktemp("object_checker"))


def moved_set(mats):
    """eight ids of the default scene: index 0 and the last index, and at least one Lambert, metal, dielectric and emissive sphere"""
    n = len(mats)
    emissive = [i for i in range(n) if (mats["emissive"][i] > 0).any()]
    ids = [0, n - 1, emissive[0]]
    for kind in (LAMBERT, METAL, DIELECTRIC):
        ids.append(next(i for i in range(1, n - 1) if mats["type"][i] == kind and i not in ids))
    ids += [i for i in range(1, n - 1) if i not in ids][:8 - len(ids)]
    assert len(ids) == len(set(ids)) == 8 and 0 in ids and n - 1 in ids and n == 46
    for kind in (LAMBERT, METAL, DIELECTRIC):
        assert any(mats["type"][i] == kind for i in ids), kind
    assert any((mats["emissive"][i] > 0).any() for i in ids)
    return ids  # (not sorted: the table's slots are in ascending index whatever the caller's order)


def moved_centres(spheres, ids, n, seed=1):
    """each moved sphere's own centre plus a seeded offset per frame of up to +-0.3 per axis -> float32 (n, K, 3)"""
    rng = np.random.default_rng(seed)
    base = np.stack([spheres["cx"][ids], spheres["cy"][ids], spheres["cz"][ids]], axis=-1).astype(np.float32).reshape(len(ids), 3)
    return (base[None] + rng.uniform(-0.3, 0.3, (n, len(ids), 3)).astype(np.float32)).astype(np.float32)


def scene_of(spheres, ids, centres, j):
    """S_j: the spheres with the centres of the moved ids replaced by frame j's"""
    s = spheres.copy()
    for k, i in enumerate(ids):
        s["cx"][i], s["cy"][i], s["cz"][i] = centres[j, k]
    return s


def guarded_ids(n, h, w):
    import torch
    return torch.full((n + 2, h, w), -9, dtype=torch.int32, device="cuda")


def draw_keyframe_clip(tpt, w, h, scene, views, ids, centres, first=0, flags=FLAG_PROGRESSIVE, outputs=ALL, prev=None, cameras=True):
    """one tptDrawDeviceKeyframeClip call over `scene` (spheres, materials: set first) on a tile and a moments plane with previous
    contents -> dict of device tensors: tile, moments, the requested per-frame outputs (untouched sentinel planes for those not
    requested), objects, rays (a list) and cams.  Guard planes around every buffer are checked."""
    import torch
    n = len(views)
    tile0, mo0 = prev if prev is not None else previous(w, h)
    tile, mo = guarded(1, h, w, tile0[None]), guarded(1, h, w, mo0[None])
    per = {k: guarded(n, h, w) for k in OUTPUTS[:4]}
    objects = guarded_ids(n, h, w)
    rays = torch.full((n + 2,), -9, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    tpt.set_scene(*scene)
    tpt.UpdateTest(0.0, first, w, h, flags)  # (the call refuses a size no tptUpdate has seen)
    r0 = tpt.ray_counter_read()
    ptr = lambda k: per[k][1].data_ptr() if k in outputs else None  # noqa: E731
    cams = tpt.draw_device_keyframe_clip(views, ids, centres, first, w, h, tile[1].data_ptr(), mo[1].data_ptr(), flags,
                                         images_ptr=ptr("images"), albedo_ptr=ptr("albedo"), normal_depth_ptr=ptr("nd"),
                                         frame_moments_ptr=ptr("fmo"), rays_ptr=rays[1:].data_ptr() if "rays" in outputs else None,
                                         objects_ptr=objects[1].data_ptr() if "objects" in outputs else None, cameras=cameras)
    total = tpt.ray_counter_read() - r0
    torch.cuda.synchronize()
    for name, t in list(per.items()) + [("tile", tile), ("moments", mo)]:
        assert guards_intact(t), "the call wrote outside %s" % name
        if name in OUTPUTS and name not in outputs:
            assert bool((t == GUARD).all()), "the call wrote %s, which was not requested" % name
    assert bool((objects[0] == -9).all()) and bool((objects[-1] == -9).all()), "the call wrote outside the object planes"
    if "objects" not in outputs:
        assert bool((objects == -9).all()), "the call wrote the object planes, which were not requested"
    r = rays.cpu().tolist()
    assert r[0] == -9 and r[-1] == -9
    if "rays" in outputs:
        assert total == sum(r[1:-1]), (total, r)
    else:
        assert r == [-9] * (n + 2)
    assert (cams is None) == (not cameras)
    out = {k: per[k][1:n + 1] for k in per}
    out.update(tile=tile[1], moments=mo[1], rays=r[1:-1], total=total, cams=cams, objects=objects[1:n + 1])
    return out


def draw_keyframe_sequence(tpt, w, h, scene, views, ids, centres, first=0, flags=FLAG_PROGRESSIVE, prev=None):
    """the same frames as tptSetScene(S_j) + tptSetCamera + tptUpdate + tptDrawDeviceMoments per frame on buffers with the same previous
    contents; the camera from tptGetSceneDesc and the object plane from tptObjectPlaneDevice right after each tptUpdate -> the same dict"""
    import torch
    n = len(views)
    spheres, mats = scene
    tile0, mo0 = prev if prev is not None else previous(w, h)
    tile, mo = torch.from_numpy(tile0).cuda(), torch.from_numpy(mo0).cuda()
    out = {k: torch.full((n, h, w, 4), GUARD, dtype=torch.float32, device="cuda") for k in OUTPUTS[:4]}
    objects = torch.full((n, h, w), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rays, cams = [], []
    for j in range(n):
        v = [float(x) for x in views[j]]
        tpt.set_scene(scene_of(spheres, ids, centres, j), mats)
        tpt.set_camera(v[0:3], v[3:6], v[6], v[7], v[8])
        tpt.UpdateTest(0.0, first + j, w, h, flags)
        cams.append(tpt.GetSceneDesc()[2].copy())
        tpt.object_plane_device(w, h, objects[j].data_ptr(), cameras=cams[-1])
        r0 = tpt.ray_counter_read()
        tpt.draw_device_moments(0.0, first + j, w, h, tile.data_ptr(), mo.data_ptr(), flags, albedo_ptr=out["albedo"][j].data_ptr(),
                                normal_depth_ptr=out["nd"][j].data_ptr())
        rays.append(tpt.ray_counter_read() - r0)  # (synchronises: the tile and the moments hold frame j)
        out["images"][j].copy_(tile)
        out["fmo"][j].copy_(mo)
    torch.cuda.synchronize()
    out.update(tile=tile, moments=mo, rays=rays, total=sum(rays), cams=np.concatenate(cams), objects=objects)
    return out


def assert_same_all(a, b, what):
    import torch
    assert_same(a, b, what)
    assert a["cams"].dtype == b["cams"].dtype and a["cams"].tobytes() == b["cams"].tobytes(), "the cameras differ from " + what
    for j in range(a["objects"].shape[0]):
        assert torch.equal(a["objects"][j], b["objects"][j]), "frame %d: the object plane differs from %s" % (j, what)


def assert_same_as_sequence(tpt, w, h, scene, views, ids, centres, first=0, flags=FLAG_PROGRESSIVE):
    a = draw_keyframe_clip(tpt, w, h, scene, views, ids, centres, first, flags)
    tpt.set_camera(None)
    b = draw_keyframe_sequence(tpt, w, h, scene, views, ids, centres, first, flags)
    assert_same_all(a, b, "the tptSetScene + tptSetCamera + tptUpdate + tptDrawDeviceMoments sequence")
    return a


def default_case(tpt, n, seed=1):
    spheres, mats = tpt.GetSceneDesc()[:2]
    ids = moved_set(mats)
    return (spheres, mats), orbit_views(n), ids, moved_centres(spheres, ids, n, seed)


def count_launches(tpt, w, h, scene, views, ids, centres, flags=FLAG_PROGRESSIVE):
    import torch
    n = len(views)
    tile, mo = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tpt.set_scene(*scene)
    tpt.UpdateTest(0.0, 0, w, h, flags)
    tpt.kernel_timing_begin(2 * n)
    tpt.draw_device_keyframe_clip(views, ids, centres, 0, w, h, tile.data_ptr(), mo.data_ptr(), flags)
    ms, launches = tpt.kernel_timing_end()
    assert ms > 0.0
    return launches


# ---------------------------------------------------------------- 1. against the sequence
@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("flags", [FLAG_PROGRESSIVE, 0], ids=["progressive", "each-frame-its-own"])
@pytest.mark.parametrize("n", [3, 33, 65])
def test_clip_equals_the_sequence(tpt_defaults, n, flags, first):
    """44 x 20: neither dimension a multiple of 8.  33 frames: two launches; 65: three, the staging's alternating halves reused"""
    tpt = tpt_defaults
    w, h = 44, 20
    scene, views, ids, centres = default_case(tpt, n)
    got = assert_same_as_sequence(tpt, w, h, scene, views, ids, centres, first, flags)
    assert np.array_equal(got["moments"][..., 3].cpu().numpy(), previous(w, h)[1][..., 3])  # (the moments' .w is nobody's to write)


# ---------------------------------------------------------------- 2. against the independent CPU statement
@pytest.mark.parametrize("flags", [FLAG_PROGRESSIVE, 0], ids=["progressive", "each-frame-its-own"])
def test_three_frames_equal_the_checker(tpt_defaults, checker, oracle, flags):
    """32 x 16 x 4, three frames, each over its own spheres S_j through the oracle's camera.  A kernel that traced every frame over one
    frame's centres must not pass: the test first asserts, with the checker alone, that frame 1 rendered with frame 0's centres differs
    from frame 1's own normal / depth plane in at least 16 pixels."""
    tpt = tpt_defaults
    w, h, n = 32, 16, 3
    spheres, mats = tpt.GetSceneDesc()[:2]  # (the default scene, with its derived data)
    assert spheres[["cx", "cy", "cz", "radius"]].tobytes() == oracle.default_scene()[0][["cx", "cy", "cz", "radius"]].tobytes()
    views = orbit_views(n)
    ids = moved_set(mats)
    centres = moved_centres(spheres, ids, n)
    bb, mo = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    want = []
    for j in range(n):
        cam = oracle_cam(oracle, views[j], w, h)
        r, _, _, alb, nd = checker.render(scene_of(spheres, ids, centres, j), mats, cam, w, h, 4, j, flags, backbuffer=bb, moments=mo)
        want.append((r, bb.copy(), mo.copy(), alb, nd, cam))
        if j == 1:
            nd_prev = checker.render(scene_of(spheres, ids, centres, 0), mats, cam, w, h, 4, 1, flags)[4]
            differ = int((nd.view(np.int32) != nd_prev.view(np.int32)).any(axis=-1).sum())
            assert differ >= 16, ("frame 0's centres", differ)
    zeros = (np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32))
    got = draw_keyframe_clip(tpt, w, h, (spheres, mats), views, ids, centres, 0, flags, prev=zeros)
    for j in range(n):
        r, image, moments, alb, nd, cam = want[j]
        assert got["rays"][j] == r, (j, got["rays"][j], r)
        assert got["cams"][j].tobytes() == cam.tobytes(), "frame %d: the camera differs from the oracle's" % j
        for k, ref in (("images", image), ("fmo", moments), ("albedo", alb), ("nd", nd)):
            assert got[k][j].cpu().numpy().tobytes() == ref.tobytes(), "frame %d: %s differs from the checker" % (j, k)
    assert got["tile"].cpu().numpy().tobytes() == bb.tobytes() and got["moments"].cpu().numpy().tobytes() == mo.tobytes()


# ---------------------------------------------------------------- 3. against the camera clip
def test_spheres_1_and_8_equal_the_animated_camera_clip(tpt_defaults, oracle):
    """ids (1, 8) at the centres the reference's rule gives at irregular times, flags 0, against tptDrawDeviceCameraClip with kFlagAnimate
    at those times: the same per-frame outputs and rays (without the progressive flag the lerp factor is 0 either way)"""
    tpt = tpt_defaults
    w, h, n = 44, 20, 33
    times, views = irregular_times(n, seed=3), orbit_views(n)
    spheres, mats = tpt.GetSceneDesc()[:2]
    centres = np.zeros((n, 2, 3), np.float32)
    moved = spheres.copy()
    for j, t in enumerate(times):
        oracle.animate(moved, t)
        for k, i in enumerate((1, 8)):
            centres[j, k] = (moved["cx"][i], moved["cy"][i], moved["cz"][i])
    a = draw_keyframe_clip(tpt, w, h, (spheres, mats), views, [1, 8], centres, 2, 0)
    tpt.set_scene(None)
    tpt.set_camera(None)
    b = draw_camera_clip(tpt, w, h, times, views, 2, FLAG_ANIMATE)
    assert a["rays"] == b["rays"]
    for k in OUTPUTS[:4]:
        for j in range(n):
            assert same(a[k][j], b[k][j]), "frame %d: %s differs from the animated camera clip" % (j, k)
    assert a["cams"].tobytes() == b["cams"].tobytes()


def test_nothing_moved_equals_the_static_camera_clip(tpt_defaults):
    """nMoved == 0 with the progressive flag against the camera clip without kFlagAnimate: everything, the tile included"""
    tpt = tpt_defaults
    w, h, n = 44, 20, 33
    views = orbit_views(n)
    scene = tpt.GetSceneDesc()[:2]
    a = draw_keyframe_clip(tpt, w, h, scene, views, [], np.zeros((n, 0, 3), np.float32), 1, FLAG_PROGRESSIVE, outputs=OUTPUTS)
    tpt.set_scene(None)
    tpt.set_camera(None)
    b = draw_camera_clip(tpt, w, h, [0.0] * n, views, 1, FLAG_PROGRESSIVE)
    assert_same(a, b, "the camera clip in which nothing moves")
    assert a["cams"].tobytes() == b["cams"].tobytes()


# ---------------------------------------------------------------- 4. launch counts, and the calls that go frame by frame
def test_one_trace_launch_per_32_frames(tpt_defaults):
    tpt = tpt_defaults
    for n in (1, 32, 33, 65):
        scene, views, ids, centres = default_case(tpt, n)
        assert count_launches(tpt, 44, 20, scene, views, ids, centres) == (n + 31) // 32, n
        assert tpt.launch_info()["blocks_per_cu"] == 2, tpt.launch_info()  # (the LDS of the single-frame twin)
        tpt.set_scene(None)


def stress_views(n):
    from toypathtracer_amd.scenes import STRESS_CAMERA
    c = STRESS_CAMERA
    return orbit_views(n, height=c["look_from"][1], radius=c["look_from"][2], focus=c["focus_dist"])


def test_flat_scene_of_200_spheres(tpt_defaults):
    """a flat scene whose arrays stay in global memory (the kernel instantiated without the scene in LDS), ids up to 63, one of them a
    light: one launch per 32 frames, the sequence's bytes"""
    tpt = tpt_defaults
    s, m = flat_scene()
    tpt.set_scene(s, m)
    spheres, mats = tpt.GetSceneDesc()[:2]
    ids = [63, 2, 17, 40, 0, 5, 62, 31]
    assert (mats["emissive"][2] > 0).any()
    for n in (1, 32, 33, 65):
        assert count_launches(tpt, 44, 20, (spheres, mats), stress_views(n), ids, moved_centres(spheres, ids, n, seed=2)) == (n + 31) // 32, n
    w, h, n = 44, 20, 33
    assert_same_as_sequence(tpt, w, h, (spheres, mats), stress_views(n), ids, moved_centres(spheres, ids, n, seed=2), 1)
    info = tpt.scene_info()
    assert info["spheres"] == 200 and info["groups"] == 0, info
    tpt.set_scene(None)


@pytest.mark.parametrize("case", ["id-64", "nine-moved", "256-spheres"])
def test_fallbacks_go_frame_by_frame(tpt_defaults, case):
    """an id of 64 on the 200-sphere scene, nine moved spheres, and a grouped scene: the single-frame moments kernel with the spheres and
    the camera set per frame, one launch per frame, the same bytes"""
    from toypathtracer_amd.scenes import stress_scene
    tpt = tpt_defaults
    w, h, n = 32, 16, 3
    if case == "id-64":
        tpt.set_scene(*flat_scene())
        ids, views = [3, 64], stress_views(n)
    elif case == "nine-moved":
        ids, views = [0, 45, 1, 2, 3, 4, 5, 6, 7], orbit_views(n)
    else:
        tpt.set_scene(*stress_scene(256, 16))
        ids, views = [1, 200], stress_views(n)
    spheres, mats = tpt.GetSceneDesc()[:2]
    centres = moved_centres(spheres, ids, n, seed=3)
    assert_same_as_sequence(tpt, w, h, (spheres, mats), views, ids, centres)
    assert count_launches(tpt, w, h, (spheres, mats), views, ids, centres) == n
    assert tpt.scene_info()["spheres"] == {"id-64": 200, "nine-moved": 46, "256-spheres": 256}[case]
    tpt.set_scene(None)


# ---------------------------------------------------------------- 5. optional outputs
@pytest.mark.parametrize("only", list(ALL) + ["none"])
def test_optional_outputs(tpt_defaults, only):
    """each of the six per-frame outputs alone, and none of them (outCameras NULL as well): what is asked for is what the call with
    every output gives, nothing else is written (draw_keyframe_clip checks the guard planes and that an output not asked for stays
    untouched)"""
    import torch
    tpt = tpt_defaults
    w, h, n = 44, 20, 34
    scene, views, ids, centres = default_case(tpt, n, seed=6)
    full = draw_keyframe_clip(tpt, w, h, scene, views, ids, centres, 1)
    tpt.set_camera(None)
    outputs = () if only == "none" else (only,)
    part = draw_keyframe_clip(tpt, w, h, scene, views, ids, centres, 1, outputs=outputs, cameras=only != "none")
    assert_same(part, full, "the call with every output", outputs)
    if only == "objects":
        assert torch.equal(part["objects"], full["objects"])
    if only != "none":
        assert part["cams"].tobytes() == full["cams"].tobytes()


# ---------------------------------------------------------------- 6. the object planes
def test_object_planes_equal_the_oracle(tpt_defaults, object_checker):
    """plane j is the oracle's HitSpheres for the centre ray of frame j's camera over S_j, and what tptObjectPlaneDevice gives inside
    the sequence; the moved spheres show in it and the planes differ from frame to frame"""
    import torch
    tpt = tpt_defaults
    w, h, n = 44, 20, 34
    scene, views, ids, centres = default_case(tpt, n, seed=4)
    a = draw_keyframe_clip(tpt, w, h, scene, views, ids, centres)
    got = a["objects"].cpu().numpy()
    for j in range(n):
        want = object_checker.plane(scene_of(scene[0], ids, centres, j), a["cams"][j:j + 1], w, h)
        assert got[j].tobytes() == want[0].tobytes(), "frame %d: the object plane differs from the oracle's HitSpheres" % j
    assert np.isin(got, ids).any() and (got == -1).any() and got[0].tobytes() != got[1].tobytes()
    tpt.set_camera(None)
    b = draw_keyframe_sequence(tpt, w, h, scene, views, ids, centres)
    assert torch.equal(a["objects"], b["objects"])


# ---------------------------------------------------------------- 7. the context afterwards
def test_the_context_afterwards(tpt_defaults, oracle):
    """tptGetSceneDesc's spheres are S_{n-1} and its camera the last view's; the next tptDrawDevice without a tptUpdate draws what it
    draws after the sequence; tptObjectPlaneDevice without cameras gives the last frame's plane"""
    import torch
    tpt = tpt_defaults
    w, h, n = 44, 20, 34
    scene, views, ids, centres = default_case(tpt, n, seed=2)

    def after(out):
        s, _, cam, _ = tpt.GetSceneDesc()
        desc = (s.copy(), cam.copy())
        plane = torch.full((h, w), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        tpt.object_plane_device(w, h, plane.data_ptr())
        tpt.draw_device(0.0, n, w, h, out["tile"].data_ptr(), FLAG_PROGRESSIVE)
        tpt.synchronize()
        return desc, plane

    a = draw_keyframe_clip(tpt, w, h, scene, views, ids, centres)
    (sa, ca), pa = after(a)
    tpt.set_camera(None)
    b = draw_keyframe_sequence(tpt, w, h, scene, views, ids, centres)
    (sb, cb), pb = after(b)
    torch.cuda.synchronize()
    assert ca.tobytes() == cb.tobytes() == a["cams"][-1].tobytes() == oracle_cam(oracle, views[-1], w, h).tobytes()
    assert sa.tobytes() == sb.tobytes() == scene_of(scene[0], ids, centres, n - 1).tobytes()
    assert same(a["tile"], b["tile"]), "tptDrawDevice after the call differs from tptDrawDevice after the sequence"
    assert torch.equal(pa, pb) and torch.equal(pa, a["objects"][-1])


# ---------------------------------------------------------------- 8. the chain the planes, the cameras and the object planes are made for
def test_planes_feed_the_object_following_temporal_pass(tpt_defaults):
    """frames 1 and 2 of ONE call without the progressive flag through tptTemporalAccumulateObjectsDevice with the call's cameras and
    object planes and api.motion_table(S_1, S_2): the bytes the pass gives on the sequence's planes, finite, and strictly more pixels
    of the moved spheres reach N == 2 than through tptTemporalAccumulateDevice on the same planes"""
    import torch
    tpt = tpt_defaults
    w, h, n, flags = 44, 20, 3, 0
    scene, views, ids, centres = default_case(tpt, n, seed=5)
    table = tpt.motion_table(scene_of(scene[0], ids, centres, 1), scene_of(scene[0], ids, centres, 2), 0.0)
    assert np.count_nonzero(table[:, :3].any(axis=1)) == len(ids)
    zeros = (np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32))
    nan_planes = lambda: [torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in range(4)]  # noqa: E731

    def chain(src, follow=True):
        planes = lambda j: (src["images"][j], src["albedo"][j], src["nd"][j], src["fmo"][j])  # noqa: E731
        first, second = nan_planes(), nan_planes()
        motion = torch.from_numpy(table).cuda()
        torch.cuda.synchronize()
        if follow:
            tpt.temporal_accumulate_objects_device(w, h, src["cams"][1], *[t.data_ptr() for t in planes(1)], src["objects"][1].data_ptr(),
                                                   *[t.data_ptr() for t in first])
            prev = (src["cams"][1], first[0].data_ptr(), first[1].data_ptr(), planes(1)[2].data_ptr(), first[2].data_ptr(),
                    src["objects"][1].data_ptr())
            tpt.temporal_accumulate_objects_device(w, h, src["cams"][2], *[t.data_ptr() for t in planes(2)], src["objects"][2].data_ptr(),
                                                   *[t.data_ptr() for t in second], prev=prev, motion_ptr=motion.data_ptr(),
                                                   n_objects=table.shape[0])
        else:
            tpt.temporal_accumulate_device(w, h, src["cams"][1], *[t.data_ptr() for t in planes(1)], *[t.data_ptr() for t in first])
            prev = (src["cams"][1], first[0].data_ptr(), first[1].data_ptr(), planes(1)[2].data_ptr(), first[2].data_ptr())
            tpt.temporal_accumulate_device(w, h, src["cams"][2], *[t.data_ptr() for t in planes(2)], *[t.data_ptr() for t in second], prev=prev)
        tpt.synchronize()
        return first + second

    got = draw_keyframe_clip(tpt, w, h, scene, views, ids, centres, 0, flags, prev=zeros)
    a = chain(got)
    plain = chain(got, follow=False)
    tpt.set_camera(None)
    b = chain(draw_keyframe_sequence(tpt, w, h, scene, views, ids, centres, 0, flags, prev=zeros))
    assert all(same(x, y) for x, y in zip(a, b))
    assert all(bool(torch.isfinite(x[..., :3]).all()) for x in a)
    on = np.isin(got["objects"][2].cpu().numpy(), ids)
    followed = int((a[6].cpu().numpy()[..., 3][on] == 2).sum())
    lost = int((plain[6].cpu().numpy()[..., 3][on] == 2).sum())
    print("the moved spheres cover %d pixels; N == 2 on them: followed %d, plain pass %d" % (int(on.sum()), followed, lost))
    assert followed > lost


# ---------------------------------------------------------------- 9. refusals on the device
def test_refusals_write_nothing(tpt_defaults):
    import torch
    tpt = tpt_defaults
    lib = tpt.load_library()
    w, h, n = 44, 20, 3
    scene, views, ids, centres = default_case(tpt, n)
    tile, mo = guarded(1, h, w), guarded(1, h, w)
    per = [guarded(n, h, w) for _ in range(4)]
    objects = guarded_ids(n, h, w)
    rays = torch.full((n,), -9, dtype=torch.int64, device="cuda")
    cams = np.full(n * 88, 0xA5, np.uint8)
    torch.cuda.synchronize()
    tpt.UpdateTest(0.0, 0, w, h, 0)
    before = [a.tobytes() for a in tpt.GetSceneDesc()]
    count = [0]

    def refused(what, ids_=ids, c=centres, flags=FLAG_PROGRESSIVE, ob=objects[1].data_ptr(), im=per[0][1].data_ptr()):
        i32 = np.ascontiguousarray(ids_, np.int32)
        c32 = np.ascontiguousarray(c, np.float32)
        vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        rc = lib.tptDrawDeviceKeyframeClip(0, n, views.ctypes.data, len(i32), i32.ctypes.data, c32.ctypes.data, w, h, vp(tile[1].data_ptr()),
                                           vp(mo[1].data_ptr()), vp(im), vp(per[1][1].data_ptr()), vp(per[2][1].data_ptr()),
                                           vp(per[3][1].data_ptr()), vp(rays.data_ptr()), vp(ob), cams.ctypes.data, flags)
        msg = lib.tptGetLastError().decode()
        assert rc != 0 and "tptDrawDeviceKeyframeClip" in msg, (what, rc, msg)
        tpt.synchronize()
        torch.cuda.synchronize()
        assert all(bool((t == GUARD).all()) for t in [tile, mo] + per), "a refused call wrote a plane: " + what
        assert bool((objects == -9).all()) and bool((rays == -9).all()) and (cams == 0xA5).all(), "a refused call wrote: " + what
        assert [a.tobytes() for a in tpt.GetSceneDesc()] == before, "a refused call changed the scene or the camera: " + what
        count[0] += 1

    refused("a repeated id", ids_=ids[:7] + ids[:1])
    bad = centres.copy()
    bad[2, 5, 1] = np.nan
    refused("a NaN centre", c=bad)
    bad[2, 5, 1] = np.inf
    refused("an infinite centre", c=bad)
    refused("kFlagAnimate", flags=FLAG_PROGRESSIVE | FLAG_ANIMATE)
    refused("an unknown flag bit", flags=4)
    refused("an id of 46", ids_=ids[:7] + [46])
    refused("the object planes start in the images' last plane", ob=per[0][1].data_ptr() + 3 * w * h * 16 - 4)
    refused("the images start in the object planes' last plane", im=objects[1].data_ptr() + 3 * w * h * 4 - 16)
    assert count[0] == 8
