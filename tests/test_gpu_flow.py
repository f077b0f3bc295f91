"""tptMotionVectorsDevice on the GPU.  Every byte of the output is held (no tolerance anywhere) against the CPU statement
(tests/flow_checker.c): on synthetic planes that differ per frame, in both forms, with and without tables and the prev set; and on a
real keyframe clip -- a 0.5-degree orbit with one sphere moved.  On that clip the call agrees with the temporal passes about where a
history exists, nothing moving gives zero motion, the object form follows the moved sphere, and a clip cut in two gives the bytes of one
call.  Refused calls write nothing."""
import ctypes as C

import numpy as np
import pytest

from clip_denoise_lib import camera_records
from flow_lib import FORMS, KINDS, TOLERANCES, FlowChecker, synthetic_clip
from test_gpu_animation_moments import GUARD
from test_gpu_camera_clip import orbit_views
from test_gpu_keyframe_clip import draw_keyframe_clip, scene_of

pytestmark = pytest.mark.gpu

MOVED = 8          # the small Lambert sphere that floats left of the scene's middle, nothing in front of it
STEP = 0.25        # what it moves per frame along x: most of its radius (0.3), about three pixels at 96 x 54


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return FlowChecker(tmp_path_factory.mktemp("flow_checker"))


def upload(clip):
    """a host clip (flow_lib.synthetic_clip's layout) -> the same dict with device tensors, and `host`, the clip itself"""
    import torch
    dev = {k: torch.from_numpy(np.ascontiguousarray(clip[k])).cuda() for k in ("albedo", "nd", "objects", "motion")}
    dev["prev"] = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in clip["prev"][1:]) if clip.get("prev") else None
    dev["host"] = clip
    return dev


def motion_vectors(tpt, dev, objects=True, table=True, prev=True, first=0, count=None, prev_from=None, **tol):
    """one motion_vectors_device call over frames first .. first + count - 1 of the device clip -> float32 [count, h, w, 4] on the host.
    prev: the clip's own prev set; prev_from = j: the prev set is plane j and camera j of the clip.  The output stack is pre-filled with
    a sentinel and followed by a guard plane, which must stay untouched; no input may change."""
    import torch
    host = dev["host"]
    n, h, w = host["albedo"].shape[:3]
    count = n - first if count is None else count
    cams = camera_records(tpt, host["cameras"])
    out = torch.full((count + 1, h, w, 4), GUARD, dtype=torch.float32, device="cuda")
    watched = [dev[k] for k in ("albedo", "nd", "objects", "motion")] + list(dev["prev"] or ())
    before = [t.clone() for t in watched]
    pv = None
    if prev_from is not None:
        j = prev_from
        pv = (cams[j], dev["albedo"][j].data_ptr(), dev["nd"][j].data_ptr()) + ((dev["objects"][j].data_ptr(),) if objects else ())
    elif prev:
        pcam = camera_records(tpt, host["prev"][0])[0]
        pv = (pcam, dev["prev"][0].data_ptr(), dev["prev"][1].data_ptr()) + ((dev["prev"][2].data_ptr(),) if objects else ())
    use_table = objects and table
    torch.cuda.synchronize()
    tpt.motion_vectors_device(w, h, count, dev["albedo"][first].data_ptr(), dev["nd"][first].data_ptr(), out.data_ptr(),
                              cams[first:first + count], objects_ptr=dev["objects"][first].data_ptr() if objects else None,
                              motion_ptr=dev["motion"][first].data_ptr() if use_table else None,
                              n_objects=host["motion"].shape[1] if use_table else 0, prev=pv, **tol)
    tpt.synchronize()
    torch.cuda.synchronize()
    assert bool((out[count] == GUARD).all()), "the call wrote behind deviceFrameMotion"
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(watched, before)), "the call wrote an input"
    return out[:count].cpu().numpy()


def assert_frames(got, want, what):
    for j in range(got.shape[0]):
        bad = got[j].view(np.uint32) != want[j].view(np.uint32)
        assert not bad.any(), "%s: frame %d differs from the CPU statement in %d words, first at %r" % (what, j, int(bad.sum()), tuple(np.argwhere(bad)[0]))


# ---------------------------------------------------------------- 1. synthetic planes that differ per frame
@pytest.mark.parametrize("size", [(1, 1), (65, 5), (130, 67)], ids=lambda s: "%dx%d" % s)
def test_synthetic_clips_equal_the_checker(tpt_defaults, checker, size):
    """three frames with three different cameras and planes (so a wrong frame index, or a tap taken from a neighbouring plane, changes
    bytes), with and without the prev set, both forms, with and without a table, at the tolerances whose edges the clips plant"""
    tpt = tpt_defaults
    w, h = size
    for kind in KINDS:
        clip = synthetic_clip(kind, w, h)
        dev = upload(clip)
        for form in FORMS:
            for prev in (True, False):
                got = motion_vectors(tpt, dev, prev=prev, **form, **TOLERANCES)
                assert_frames(got, checker.run(clip, prev=prev, **form, **TOLERANCES), "%s %r prev=%s" % (kind, form, prev))
    got = motion_vectors(tpt, dev, **FORMS[2])  # (the binding's default tolerances)
    assert_frames(got, checker.run(clip, **FORMS[2], **{k: v for k, v in tpt.TEMPORAL_DEFAULTS.items() if k != "max_history"}), "defaults")


# ---------------------------------------------------------------- 2. a real clip
REAL = {}


def real_clip(tpt):
    """96 x 54 x 4 spp, 5 frames of tptDrawDeviceKeyframeClip over the default scene: a 0.5-degree orbit, sphere MOVED moved by STEP
    per frame; api.motion_table tables (caps 0).  Drawn once -> the device clip of upload(), the spheres of every frame, the scene"""
    if REAL:
        return REAL
    w, h, n = 96, 54, 5
    spheres, mats = tpt.GetSceneDesc()[:2]
    centres = np.array([[[spheres["cx"][MOVED] + np.float32(STEP) * j, spheres["cy"][MOVED], spheres["cz"][MOVED]]] for j in range(n)],
                       np.float32)
    zero = (np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32))
    src = draw_keyframe_clip(tpt, w, h, (spheres, mats), orbit_views(n, step=0.5), [MOVED], centres, 0, 0, prev=zero)
    tables = [np.zeros((len(spheres), 4), np.float32)]
    for j in range(1, n):
        tables.append(tpt.motion_table(scene_of(spheres, [MOVED], centres, j - 1), scene_of(spheres, [MOVED], centres, j)))
    assert all(t[MOVED, 0] == -np.float32(STEP) and np.count_nonzero(t) == 1 for t in tables[1:])
    clip = dict(cameras=np.ascontiguousarray(src["cams"]).view(np.float32).reshape(n, 22).copy(), albedo=src["albedo"].cpu().numpy(),
                nd=src["nd"].cpu().numpy(), objects=src["objects"].cpu().numpy(), motion=np.ascontiguousarray(np.stack(tables)), prev=None)
    assert all(int((clip["objects"][j] == MOVED).sum()) > 20 for j in range(n)), "the moved sphere is not in view"
    REAL.update(w=w, h=h, n=n, dev=upload(clip), clip=clip, colour=src["images"].contiguous(), moments=src["fmo"].contiguous(),
                cams=src["cams"], scene=(spheres, mats))
    return REAL


def defaults(tpt):
    return {k: v for k, v in tpt.TEMPORAL_DEFAULTS.items() if k != "max_history"}


def test_a_real_clip_equals_the_checker(tpt_defaults, checker):
    tpt = tpt_defaults
    R = real_clip(tpt)
    for form in FORMS:
        got = motion_vectors(tpt, R["dev"], prev=False, count=4, **form)
        want = checker.run({k: (v[:4] if isinstance(v, np.ndarray) else v) for k, v in R["clip"].items()}, prev=False, **form, **defaults(tpt))
        assert_frames(got, want, "the keyframe clip %r" % form)
        assert not got[0].any() and (got[1:, ..., 3] > 0).mean() > 0.5 and (got[1:, ..., 3] == 0).any()
        assert np.abs(got[1:, ..., 0]).max() > 0.25, "an orbit of 0.5 degrees moves some pixel by more than a quarter"


def test_weight_agrees_with_the_temporal_passes(tpt_defaults):
    """frames 0 and 1 of the clip: frame 0 through the pass as a first frame, frame 1 with maxHistory = 2 -- its history length is 2
    exactly where this call's W > 0.  The tap sets are the same by construction: T_0's albedo is frame 0's own, its history length 1
    everywhere, its colour finite."""
    import torch
    tpt = tpt_defaults
    R = real_clip(tpt)
    w, h, dev, cams = R["w"], R["h"], R["dev"], R["cams"]
    assert bool(torch.isfinite(R["colour"][0]).all())
    for objects in (False, True):
        t0, t1 = (tuple(torch.full((h, w, 4), GUARD, dtype=torch.float32, device="cuda") for _ in range(4)) for _ in range(2))
        cur = lambda j: (R["colour"][j].data_ptr(), dev["albedo"][j].data_ptr(), dev["nd"][j].data_ptr(), R["moments"][j].data_ptr())  # noqa: E731
        kw = dict(max_history=2.0, **defaults(tpt))
        if objects:
            tpt.temporal_accumulate_objects_device(w, h, cams[0], *cur(0), dev["objects"][0].data_ptr(), *(t.data_ptr() for t in t0), **kw)
            tpt.temporal_accumulate_objects_device(
                w, h, cams[1], *cur(1), dev["objects"][1].data_ptr(), *(t.data_ptr() for t in t1),
                prev=(cams[0], t0[0].data_ptr(), t0[1].data_ptr(), dev["nd"][0].data_ptr(), t0[2].data_ptr(), dev["objects"][0].data_ptr()),
                motion_ptr=dev["motion"][1].data_ptr(), n_objects=R["clip"]["motion"].shape[1], **kw)
        else:
            tpt.temporal_accumulate_device(w, h, cams[0], *cur(0), *(t.data_ptr() for t in t0), **kw)
            tpt.temporal_accumulate_device(w, h, cams[1], *cur(1), *(t.data_ptr() for t in t1),
                                           prev=(cams[0], t0[0].data_ptr(), t0[1].data_ptr(), dev["nd"][0].data_ptr(), t0[2].data_ptr()), **kw)
        tpt.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(t0[1].view(torch.int32), dev["albedo"][0].view(torch.int32)) and bool((t0[2][..., 3] == 1).all())
        N = t1[2][..., 3].cpu().numpy()
        W = motion_vectors(tpt, dev, prev=False, count=2, **FORMS[2 if objects else 0])[1][..., 3]
        assert set(np.unique(N)) == {1.0, 2.0}
        assert ((N == 2) == (W > 0)).all(), "%d pixels disagree (objects: %s)" % (int(((N == 2) != (W > 0)).sum()), objects)


def test_nothing_moves(tpt_defaults, checker):
    """two frames of one camera and one scene: mv == {0, 0} for every pixel that projects.  (A float32 simulation of steps 1-3 with
    the default camera puts px at most 2.3e-5 from x at this size -- 4.9e-4 at 1280 x 720 -- against a snap of 1/128.)"""
    tpt = tpt_defaults
    w, h = 96, 54
    spheres, mats = tpt.GetSceneDesc()[:2]
    zero = (np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32))
    src = draw_keyframe_clip(tpt, w, h, (spheres, mats), orbit_views(2, step=0.0), [], np.zeros((2, 0, 3), np.float32), 0, 0, prev=zero)
    clip = dict(cameras=np.ascontiguousarray(src["cams"]).view(np.float32).reshape(2, 22).copy(), albedo=src["albedo"].cpu().numpy(),
                nd=src["nd"].cpu().numpy(), objects=src["objects"].cpu().numpy(), motion=np.zeros((2, 1, 4), np.float32), prev=None)
    assert clip["cameras"][0].tobytes() == clip["cameras"][1].tobytes()
    for form in FORMS[:2]:
        got = motion_vectors(tpt, upload(clip), prev=False, **form)
        assert_frames(got, checker.run(clip, prev=False, **form, **defaults(tpt)), "the still clip %r" % form)
        projects = got[1][..., 2] > 0
        assert projects.all() and (got[1][..., :2] == 0).all()
        assert (got[1][..., 3] > 0).mean() > 0.5  # (two frames of other samples: most pixels still show the same surface)


def test_the_object_form_follows_the_moved_sphere(tpt_defaults):
    tpt = tpt_defaults
    R = real_clip(tpt)
    plain = motion_vectors(tpt, R["dev"], prev=False, **FORMS[0])
    follow = motion_vectors(tpt, R["dev"], prev=False, **FORMS[2])
    on = R["clip"]["objects"][1:] == MOVED
    a, b = int((plain[1:][..., 3][on] > 0).sum()), int((follow[1:][..., 3][on] > 0).sum())
    print("pixels of the moved sphere (%d in frames 1..4) with W > 0: plain form %d, object form %d" % (int(on.sum()), a, b))
    assert b > a
    # its pixels move with it: about STEP along x in world space is about three pixels to the left of where the camera's orbit alone puts them
    assert np.median(follow[1:][..., 0][on]) < np.median(plain[1:][..., 0][on]) - 1.0


def test_a_clip_cut_in_two(tpt_defaults):
    """5 frames in one call equal calls of 2 + 3 frames with the prev set pointing at plane 1 and camera 1, byte for byte"""
    tpt = tpt_defaults
    R = real_clip(tpt)
    for form in FORMS:
        whole = motion_vectors(tpt, R["dev"], prev=False, **form)
        head = motion_vectors(tpt, R["dev"], prev=False, first=0, count=2, **form)
        tail = motion_vectors(tpt, R["dev"], first=2, count=3, prev_from=1, **form)
        assert np.concatenate([head, tail]).tobytes() == whole.tobytes(), form
        assert tail[0].any()


# ---------------------------------------------------------------- 3. refusals on the device
def test_refusals_write_nothing(tpt_defaults):
    import torch
    tpt = tpt_defaults
    lib = tpt.load_library()
    w, h, n = 65, 5, 3
    clip = synthetic_clip("moved", w, h)
    dev = upload(clip)
    out = torch.full((n, h, w, 4), GUARD, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def refused(what, **changes):
        a = tpt.MotionVectorsArgs(screenWidth=w, screenHeight=h, nFrames=n, flags=0, cameras=clip["cameras"].ctypes.data,
                                  deviceFrameAlbedo=dev["albedo"].data_ptr(), deviceFrameNormalDepth=dev["nd"].data_ptr(),
                                  deviceFrameMotion=out.data_ptr(), depthTolerance=0.1, normalTolerance=0.25, coverageTolerance=0.0)
        for k, v in changes.items():
            setattr(a, k, v)
        rc = lib.tptMotionVectorsDevice(C.byref(a))
        msg = lib.tptGetLastError().decode()
        assert rc != 0 and "tptMotionVectorsDevice" in msg, (what, rc, msg)

    refused("a flag", flags=1)
    refused("out's last plane is the first albedo plane", deviceFrameAlbedo=out.data_ptr() + 2 * w * h * 16)
    bad = clip["cameras"].copy()
    bad[2, 4] = np.inf
    refused("camera 2: a non-finite field", cameras=bad.ctypes.data)
    refused("a prev plane without prevCamera", devicePrevAlbedo=dev["prev"][0].data_ptr())
    tpt.synchronize()
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()), "a refused call wrote"
