"""The moved-sphere kernels (tptKeyframeKernel, tptCameraClipKernel, tptTraceAnimationKernel and the MOVING variants of the path-queue
kernel) across the MOTION of tests/motion_kinds_lib.py: a launch stages the scene of its last frame, and the earlier frames' spheres
leave the matrix table's range or enter it, land on another sphere, swallow the camera, take the lights 2^20 away or onto the floor, take
the ground away.  No tolerance anywhere:

  - every keyframe case: one tptDrawDeviceKeyframeClip call against the tptSetScene(S_j) + tptSetCamera + tptUpdate + tptDrawDeviceMoments
    (+ tptObjectPlaneDevice) sequence -- every frame image, albedo, normal / depth, frame moments, object plane, ray count and Camera
    record, the final tile and moments, guard planes included --, and against the CPU statement (tests/moments_checker.c over S_j, the
    oracle's object plane);
  - one case per family and every table_seam case with the scene forced into LDS and out of it;
  - the launch counts: one per 32 frames, one per frame for the three calls that go frame by frame;
  - the timed cases through tptDrawDeviceAnimation, tptDrawDeviceAnimationMoments and tptDrawDeviceCameraClip against the tptUpdate + draw
    sequence and the checker;
  - a far clip and a tie clip through tptMotionVectorsDevice and tptTemporalAccumulateObjectsDevice against their CPU statements.

tests/test_motion_kinds.py proves on the CPU what each case is and that each frame has something to show."""
import numpy as np
import pytest

import motion_kinds_lib as lib
from flow_lib import FORMS, FlowChecker
from moments_lib import MomentsChecker
from object_lib import ObjectChecker
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE
from test_gpu_animation import draw_animation, draw_sequence as draw_animation_sequence, same
from test_gpu_animation_moments import assert_same, draw_clip, draw_sequence as draw_clip_sequence
from test_gpu_camera_clip import assert_same_cameras, draw_camera_clip, draw_camera_sequence, oracle_cam
from test_gpu_flow import assert_frames, motion_vectors, upload
from test_gpu_keyframe_clip import assert_same_all, count_launches, draw_keyframe_clip, draw_keyframe_sequence
from test_motion_kinds import table_seam_of, timed_seam_x
from value_ranges_lib import FLOW_SIZE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def seam(emu):
    lib.set_table_seam(*table_seam_of(emu))
    return lib.TABLE_SEAM


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return MomentsChecker(tmp_path_factory.mktemp("moments_checker"))


@pytest.fixture(scope="module")
def object_checker(tmp_path_factory):
    return ObjectChecker(tmp_path_factory.mktemp("object_checker"))


@pytest.fixture(scope="module")
def flow_checker(tmp_path_factory):
    return FlowChecker(tmp_path_factory.mktemp("flow_checker"))


def configure(tpt, name):
    meta = lib.META[name]
    tpt.set_samples_per_pixel(meta["size"][2])
    tpt.set_config(meta["light_sampling"], 0.9, False)
    return meta["size"][:2]


def zeros(w, h):
    return np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)


_reference = {}


def reference_of(checker, object_checker, oracle, name):
    """the CPU statement of the clip on a zeroed tile and moments plane, computed once: per frame (rays, image, moments, albedo,
    normal / depth, camera, object plane)"""
    if name not in _reference:
        s, m, views, ids, centres, flags, first = lib.case(name)
        w, h, spp = lib.META[name]["size"]
        bb, mo = zeros(w, h)
        frames = []
        for j in range(len(views)):
            sj = lib.scene_of(s, ids, centres, j)
            cam = oracle_cam(oracle, views[j], w, h)
            r, _, _, alb, nd = checker.render(sj, m, cam, w, h, spp, first + j, flags, backbuffer=bb, moments=mo,
                                              light_sampling=lib.META[name]["light_sampling"])
            frames.append((r, bb.copy(), mo.copy(), alb, nd, cam, object_checker.plane(sj, cam, w, h)[0]))
        assert all(np.isfinite(f[1]).all() for f in frames), "the checker's own image is not finite: the case is no fair test"
        _reference[name] = frames
    return _reference[name]


def assert_equals_the_reference(got, frames, what):
    for j, (r, image, moments, alb, nd, cam, plane) in enumerate(frames):
        assert got["rays"][j] == r, (what, j, got["rays"][j], r)
        assert got["cams"][j].tobytes() == cam.tobytes(), "%s, frame %d: the camera differs from the oracle's" % (what, j)
        for k, ref in (("images", image), ("fmo", moments), ("albedo", alb), ("nd", nd)):
            assert got[k][j].cpu().numpy().tobytes() == ref.tobytes(), "%s, frame %d: %s differs from the checker" % (what, j, k)
        assert got["objects"][j].cpu().numpy().tobytes() == plane.tobytes(), "%s, frame %d: the object plane differs from the oracle's" % (what, j)
    assert got["tile"].cpu().numpy().tobytes() == frames[-1][1].tobytes() and got["moments"].cpu().numpy().tobytes() == frames[-1][2].tobytes(), what


# ---------------------------------------------------------------- 1. every keyframe case against the sequence
@pytest.mark.parametrize("name", list(lib.CATALOGUE))
def test_a_clip_equals_the_sequence(tpt_defaults, name):
    tpt = tpt_defaults
    w, h = configure(tpt, name)
    s, m, views, ids, centres, flags, first = lib.case(name)
    a = draw_keyframe_clip(tpt, w, h, (s, m), views, ids, centres, first, flags)
    tpt.set_camera(None)
    b = draw_keyframe_sequence(tpt, w, h, (s, m), views, ids, centres, first, flags)
    assert_same_all(a, b, "the tptSetScene + tptSetCamera + tptUpdate + tptDrawDeviceMoments sequence")
    got = tpt.GetSceneDesc()[0]
    want = lib.scene_of(s, ids, centres, len(views) - 1)
    assert all(got[k].tobytes() == want[k].tobytes() for k in ("cx", "cy", "cz", "radius")), "the context's spheres are not S_{n-1}"


# ---------------------------------------------------------------- 2. every keyframe case against the CPU statement
@pytest.mark.parametrize("name", list(lib.CATALOGUE))
def test_a_clip_equals_the_checker(tpt_defaults, checker, object_checker, oracle, name):
    tpt = tpt_defaults
    w, h = configure(tpt, name)
    s, m, views, ids, centres, flags, first = lib.case(name)
    got = draw_keyframe_clip(tpt, w, h, (s, m), views, ids, centres, first, flags, prev=zeros(w, h))
    assert_equals_the_reference(got, reference_of(checker, object_checker, oracle, name), name)


# ---------------------------------------------------------------- 3. the scene forced into LDS and out of it
@pytest.mark.parametrize("lds", [1, 0], ids=["lds-scene", "scene-in-global-memory"])
@pytest.mark.parametrize("name", lib.ONE_PER_FAMILY + lib.FAMILIES["table_seam"])
def test_the_lds_scene_forced_in_and_out(tpt_defaults, checker, object_checker, oracle, name, lds):
    tpt = tpt_defaults
    w, h = configure(tpt, name)
    tpt.set_kernel_variant(0, 3, lds)
    s, m, views, ids, centres, flags, first = lib.case(name)
    got = draw_keyframe_clip(tpt, w, h, (s, m), views, ids, centres, first, flags, prev=zeros(w, h))
    assert_equals_the_reference(got, reference_of(checker, object_checker, oracle, name), "%s, LDS scene %d" % (name, lds))


# ---------------------------------------------------------------- 4. launch counts
@pytest.mark.parametrize("name", list(lib.CATALOGUE))
def test_launch_counts(tpt_defaults, name):
    """one trace launch per 32 frames; nine moved spheres, an id of 64 and 256 spheres go frame by frame.  No case of the catalogue is
    routed frame by frame for its centres: the batched path holds every byte above."""
    tpt = tpt_defaults
    w, h = configure(tpt, name)
    s, m, views, ids, centres, flags, first = lib.case(name)
    n = len(views)
    want = n if name in lib.FALLBACKS else (n + 31) // 32
    assert count_launches(tpt, w, h, (s, m), views, ids, centres, flags) == want == lib.META[name]["launches"]


# ---------------------------------------------------------------- 5. the timed cases
def timed_case(emu, name):
    return lib.timed_seam(timed_seam_x(emu)[1]) if name == "timed_seam" else lib.timed(name)


def set_view(tpt, v):
    v = [float(x) for x in v]
    tpt.set_camera(v[0:3], v[3:6], v[6], v[7], v[8])


@pytest.mark.parametrize("name", list(lib.TIMED) + ["timed_seam"])
def test_a_timed_clip_through_the_three_calls(tpt_defaults, checker, oracle, emu, name):
    """tptDrawDeviceAnimation, tptDrawDeviceAnimationMoments and tptDrawDeviceCameraClip (the camera repeated) against the tptUpdate +
    draw sequences, and the camera clip against the checker over the spheres moved to each time"""
    tpt = tpt_defaults
    s, m, times, views, flags, first = timed_case(emu, name)
    w, h, spp = lib.SIZE
    assert all(v.tobytes() == views[0].tobytes() for v in views)
    tpt.set_samples_per_pixel(spp)
    tpt.set_scene(s, m)
    set_view(tpt, views[0])
    ta, ia, pa = draw_animation(tpt, w, h, times, first, flags)
    tpt.set_scene(s, m)
    tb, ib, pb = draw_animation_sequence(tpt, w, h, times, first, flags)
    assert pa == pb and same(ta, tb)
    for j in range(len(times)):
        assert same(ia[j], ib[j]), "tptDrawDeviceAnimation: frame %d differs from the tptUpdate + tptDrawDevice sequence" % j
    tpt.set_scene(s, m)
    a = draw_clip(tpt, w, h, times, first, flags)
    tpt.set_scene(s, m)
    b = draw_clip_sequence(tpt, w, h, times, first, flags)
    assert_same(a, b, "the tptUpdate + tptDrawDeviceMoments sequence (tptDrawDeviceAnimationMoments)")
    tpt.set_scene(s, m)
    a = draw_camera_clip(tpt, w, h, times, views, first, flags)
    tpt.set_scene(s, m)
    tpt.set_camera(None)
    b = draw_camera_sequence(tpt, w, h, times, views, first, flags)
    assert_same(a, b, "the tptSetCamera + tptUpdate + tptDrawDeviceMoments sequence (tptDrawDeviceCameraClip)")
    assert_same_cameras(a, b)
    # the checker, on a zeroed tile and moments plane
    tpt.set_scene(s, m)
    got = draw_camera_clip(tpt, w, h, times, views, first, flags, prev=zeros(w, h))
    bb, mo = zeros(w, h)
    cam = oracle_cam(oracle, views[0], w, h)
    for j, t in enumerate(times):
        sj = s.copy()
        oracle.animate(sj, t)
        r, _, _, alb, nd = checker.render(sj, m, cam, w, h, spp, first + j, flags, backbuffer=bb, moments=mo)
        assert np.isfinite(bb).all()
        assert got["rays"][j] == r, (j, got["rays"][j], r)
        assert got["cams"][j].tobytes() == cam.tobytes()
        for k, ref in (("images", bb), ("fmo", mo), ("albedo", alb), ("nd", nd)):
            assert got[k][j].cpu().numpy().tobytes() == ref.tobytes(), "frame %d (t = %r): %s differs from the checker" % (j, t, k)
    assert flags == FLAG_PROGRESSIVE | FLAG_ANIMATE


# ---------------------------------------------------------------- 6. downstream
@pytest.mark.parametrize("name", ["reach_2^20_mid", "tie_of_two_moved"])
def test_the_planes_downstream(tpt_defaults, flow_checker, object_checker, name):
    """the clip at 65 x 5 without the progressive flag: its albedo, normal / depth and object planes and its cameras through
    tptMotionVectorsDevice (the object form, the tables api.motion_table gives for the clip's centres) against tests/flow_checker.c,
    and frames 1 and 2 through tptTemporalAccumulateObjectsDevice against tests/object_checker.c, the CPU statement of that pass
    (tests/temporal_checker.c states tptTemporalAccumulateDevice, which follows no objects)"""
    import torch
    tpt = tpt_defaults
    configure(tpt, name)
    w, h = FLOW_SIZE
    s, m, views, ids, centres, _, first = lib.case(name)
    n = len(views)
    src = draw_keyframe_clip(tpt, w, h, (s, m), views, ids, centres, first, 0, prev=zeros(w, h))
    tables = [np.zeros((len(s), 4), np.float32)]
    for j in range(1, n):
        tables.append(tpt.motion_table(lib.scene_of(s, ids, centres, j - 1), lib.scene_of(s, ids, centres, j)))
    assert any(t.any() for t in tables[1:])
    clip = dict(cameras=np.ascontiguousarray(src["cams"]).view(np.float32).reshape(n, 22).copy(), albedo=src["albedo"].cpu().numpy(),
                nd=src["nd"].cpu().numpy(), objects=src["objects"].cpu().numpy(), motion=np.ascontiguousarray(np.stack(tables)), prev=None)
    tol = {k: v for k, v in tpt.TEMPORAL_DEFAULTS.items() if k != "max_history"}
    dev = upload(clip)
    for form in FORMS:
        assert_frames(motion_vectors(tpt, dev, prev=False, **form), flow_checker.run(clip, prev=False, **form, **tol), "%s %r" % (name, form))
    # the object-following temporal pass: frame 1 as a first frame, frame 2 on its outputs
    colour, fmo = src["images"].cpu().numpy(), src["fmo"].cpu().numpy()
    cur = lambda j: tuple(np.ascontiguousarray(a[j]) for a in (colour, clip["albedo"], clip["nd"], fmo))  # noqa: E731
    kw = dict(tpt.TEMPORAL_DEFAULTS)
    first_out = object_checker.run(src["cams"][1], cur(1), clip["objects"][1], **kw)
    prev = (src["cams"][1], first_out[0], first_out[1], cur(1)[2], first_out[2], clip["objects"][1])
    want = object_checker.run(src["cams"][2], cur(2), clip["objects"][2], prev=prev, motion=tables[2], **kw)
    dplanes = lambda j: (src["images"][j], src["albedo"][j], src["nd"][j], src["fmo"][j])  # noqa: E731
    out1, out2 = ([torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in range(4)] for _ in range(2))
    motion = torch.from_numpy(tables[2]).cuda()
    torch.cuda.synchronize()
    tpt.temporal_accumulate_objects_device(w, h, src["cams"][1], *[t.data_ptr() for t in dplanes(1)], src["objects"][1].data_ptr(),
                                           *[t.data_ptr() for t in out1], **kw)
    tpt.temporal_accumulate_objects_device(w, h, src["cams"][2], *[t.data_ptr() for t in dplanes(2)], src["objects"][2].data_ptr(),
                                           *[t.data_ptr() for t in out2],
                                           prev=(src["cams"][1], out1[0].data_ptr(), out1[1].data_ptr(), dplanes(1)[2].data_ptr(),
                                                 out1[2].data_ptr(), src["objects"][1].data_ptr()),
                                           motion_ptr=motion.data_ptr(), n_objects=tables[2].shape[0], **kw)
    tpt.synchronize()
    torch.cuda.synchronize()
    for k, (g1, g2) in enumerate(zip(out1, out2)):
        assert g1.cpu().numpy().tobytes() == first_out[k].tobytes(), "%s: output %d of the first frame's pass differs from the CPU statement" % (name, k)
        assert g2.cpu().numpy().tobytes() == want[k].tobytes(), "%s: output %d of the pass with a history differs from the CPU statement" % (name, k)
