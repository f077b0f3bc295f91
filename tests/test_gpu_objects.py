"""tptObjectPlaneDevice and tptTemporalAccumulateObjectsDevice on the GPU.  The object plane is held byte for byte against its C
statement (tests/object_checker.c, the oracle's HitSpheres) over the default scene at the edge sizes, clips with a camera and a time per
frame, the boundary of the animation rule, the 4096-sphere scene, equal spheres and a camera inside one; it leaves the context alone.
The pass is held byte for byte against its statement on real tptDrawDeviceMoments planes chained over several frames -- an animated
scene with tptObjectMotionTable's table, an orbit with capped mirrors and glass, the 4096-sphere scene without a table -- and on the
synthetic cases; without a table and with one id it is tptTemporalAccumulateDevice; a sphere moved with tptSetScene keeps its history
through api.motion_table where the plain pass loses it; refusals write nothing."""
import ctypes as C
import math

import numpy as np
import pytest

from object_lib import KINDS, ObjectChecker, synthetic_objects
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE
from temporal_lib import synthetic_case

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (17, 1), (1, 17), (130, 67), (8192, 2)]
NAMES = ("colour", "albedo", "moments", "variance")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return ObjectChecker(tmp_path_factory.mktemp("object_checker"))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def plane(h, w, fill=0.0):
    import torch
    return torch.full((h, w, 4), fill, dtype=torch.float32, device="cuda")


def host(planes):
    return [t.cpu().numpy() for t in planes]


def orbit(j, degrees):
    a = math.radians(degrees * j)
    return dict(look_from=(3.0 * math.sin(a), 2.0, 3.0 * math.cos(a)), look_at=(0.0, 0.0, 0.0), vfov=60.0, aperture=0.02, focus_dist=3.0)


def object_planes(tpt, w, h, n=1, **kw):
    """tptObjectPlaneDevice into n planes filled with -9 -> int32 [n, h, w] on the device"""
    import torch
    out = torch.full((n, h, w), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tpt.object_plane_device(w, h, out.data_ptr(), **kw)
    return out


def orbit_cameras(tpt, w, h, n, degrees, flags=0):
    """the cameras of an orbit as tptSetCamera + tptUpdate build them -> CAMERA_DT [n]; the context ends at the last one"""
    cams = []
    for j in range(n):
        tpt.set_camera(**orbit(j, degrees))
        tpt.UpdateTest(0.0, j, w, h, flags)
        cams.append(tpt.GetSceneDesc()[2].copy())
    return np.concatenate(cams)


# ---------------------------------------------------------------- the object plane
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_object_plane_default_scene(tpt_defaults, checker, size):
    tpt = tpt_defaults
    w, h = size
    tpt.UpdateTest(0.0, 0, w, h, 0)
    spheres, _, cam, _ = tpt.GetSceneDesc()
    want = checker.plane(spheres, cam, w, h)
    own = object_planes(tpt, w, h)  # cameras NULL: the update's
    given = object_planes(tpt, w, h, cameras=cam)
    tpt.synchronize()
    assert own.cpu().numpy().tobytes() == want.tobytes()
    assert given.cpu().numpy().tobytes() == want.tobytes()
    if size == (130, 67):
        assert {-1, 0, 7} <= set(np.unique(want).tolist())  # (sky, ground, the glass sphere)


@pytest.mark.parametrize("frames", [1, 3])
def test_object_plane_clip_with_cameras_and_times(tpt_defaults, checker, frames):
    tpt = tpt_defaults
    w, h = 130, 67
    times = np.array([0.3, 0.9, np.nan][:frames], np.float32)
    cams = orbit_cameras(tpt, w, h, frames, 5.0)
    spheres = tpt.GetSceneDesc()[0]
    got = object_planes(tpt, w, h, frames, times=times, cameras=cams, flags=FLAG_ANIMATE)
    tpt.synchronize()
    got = got.cpu().numpy()
    assert got.tobytes() == checker.plane(spheres, cams, w, h, times, FLAG_ANIMATE).tobytes()
    assert np.isin(got[0], (1, 8)).any()
    if frames == 3:
        assert got[0].tobytes() != got[1].tobytes() and not np.isin(got[2], (1, 8)).any()  # (a NaN time: its own frame only)
    # without the flag the times play no part
    still = object_planes(tpt, w, h, frames, times=times, cameras=cams, flags=FLAG_PROGRESSIVE)
    tpt.synchronize()
    assert still.cpu().numpy().tobytes() == checker.plane(spheres, cams, w, h).tobytes()


@pytest.mark.parametrize("count", [8, 9])
def test_object_plane_animation_boundary(tpt_defaults, checker, count):
    tpt = tpt_defaults
    w, h = 130, 67
    spheres, mats = tpt.GetSceneDesc()[:2]
    tpt.set_scene(spheres[:count], mats[:count])
    tpt.UpdateTest(0.0, 0, w, h, 0)
    cam = tpt.GetSceneDesc()[2]
    times = np.array([1.0, 2.0], np.float32)
    cams = np.concatenate([cam, cam])
    got = object_planes(tpt, w, h, 2, times=times, cameras=cams, flags=FLAG_ANIMATE)
    tpt.synchronize()
    got = got.cpu().numpy()
    assert got.tobytes() == checker.plane(spheres[:count], cams, w, h, times, FLAG_ANIMATE).tobytes()
    assert (got[0].tobytes() != got[1].tobytes()) == (count > 8)


@pytest.mark.parametrize("count", [4096, 301])
def test_object_plane_many_spheres(tpt_defaults, checker, count):
    from toypathtracer_amd.scenes import STRESS_CAMERA, stress_scene
    tpt = tpt_defaults
    w, h = 192, 108
    s, m = stress_scene(count, 64)
    tpt.set_scene(s, m)
    tpt.set_camera(**STRESS_CAMERA)
    tpt.UpdateTest(0.0, 0, w, h, 0)
    cam = tpt.GetSceneDesc()[2]
    got = object_planes(tpt, w, h)
    tpt.synchronize()
    got = got.cpu().numpy()
    assert got.tobytes() == checker.plane(s, cam, w, h).tobytes()
    assert len(np.unique(got)) > 100 and got.max() > count // 2
    assert tpt.scene_info()["groups"] > 0  # (grouped for the trace; the plane runs the exact loop over all spheres)


def test_object_plane_equal_spheres_and_a_camera_inside_one(tpt_defaults, checker):
    tpt = tpt_defaults
    w, h = 130, 67
    spheres, mats = tpt.GetSceneDesc()[:2]
    twice, mtwice = np.concatenate([spheres[:9], spheres[5:6], spheres[9:]]), np.concatenate([mats[:9], mats[5:6], mats[9:]])
    tpt.set_scene(twice, mtwice)
    tpt.UpdateTest(0.0, 0, w, h, 0)
    cam = tpt.GetSceneDesc()[2]
    got = object_planes(tpt, w, h)
    tpt.synchronize()
    got = got.cpu().numpy()
    assert got.tobytes() == checker.plane(twice, cam, w, h).tobytes()
    assert (got == 5).any() and not (got == 9).any()  # the same sphere at 5 and 9: the lower index wins
    tpt.set_scene(None)
    tpt.set_camera(look_from=(0.5, 1.0, 0.5), look_at=(0.0, 0.0, 0.0), vfov=60.0, aperture=0.0, focus_dist=3.0)  # the glass sphere's centre
    tpt.UpdateTest(0.0, 0, w, h, 0)
    cam = tpt.GetSceneDesc()[2]
    got = object_planes(tpt, w, h)
    tpt.synchronize()
    got = got.cpu().numpy()
    assert (got == 7).all() and got.tobytes() == checker.plane(spheres, cam, w, h).tobytes()  # (the far root)


def test_object_plane_of_a_clip_frame_equals_update_and_a_single_call(tpt_defaults):
    tpt = tpt_defaults
    w, h = 130, 67
    times = np.array([0.0, 0.7, 1.4, 2.1], np.float32)
    tpt.UpdateTest(0.0, 0, w, h, FLAG_ANIMATE)
    clip = object_planes(tpt, w, h, 4, times=times, flags=FLAG_ANIMATE)
    tpt.synchronize()
    clip = clip.cpu().numpy()
    for j, t in enumerate(times):
        tpt.UpdateTest(float(t), j, w, h, FLAG_ANIMATE)
        one = object_planes(tpt, w, h)
        tpt.synchronize()
        assert one.cpu().numpy()[0].tobytes() == clip[j].tobytes(), j
    assert len({clip[j].tobytes() for j in range(4)}) == 4


def test_object_plane_leaves_the_context_alone(tpt_defaults):
    """a synchronous caller's six progressive frames (the next ones may be traced ahead of its calls) with two object-plane calls after
    the fourth: scene, camera and look-ahead hits are what they were before the calls, and the run ends with the tile and the number of
    frames found traced ahead of the same run without them"""
    import torch
    tpt = tpt_defaults
    w, h = 128, 72

    def run(with_calls):
        tile = plane(h, w)
        torch.cuda.synchronize()
        hits0 = tpt.lookahead_hits()
        for f in range(6):
            tpt.UpdateTest(0.0, f, w, h, FLAG_PROGRESSIVE)
            tpt.draw_device(0.0, f, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
            tpt.synchronize()
            if with_calls and f == 3:
                before = [a.tobytes() for a in tpt.GetSceneDesc()] + [tpt.lookahead_hits()]
                times = np.array([0.5, 1.5], np.float32)
                a = object_planes(tpt, w, h, 2, times=times, flags=FLAG_ANIMATE | FLAG_PROGRESSIVE)
                b = object_planes(tpt, w, h, cameras=orbit_cam_record(tpt))
                tpt.synchronize()
                assert [x.tobytes() for x in tpt.GetSceneDesc()] + [tpt.lookahead_hits()] == before
                assert bool((a >= -1).all()) and bool((b >= -1).all()) and a[0].cpu().numpy().tobytes() != a[1].cpu().numpy().tobytes()
        return tile.cpu().numpy().tobytes(), tpt.lookahead_hits() - hits0

    assert run(True) == run(False)


def orbit_cam_record(tpt):
    """a camera that is not the context's, made without touching the context: the context's own record with its origin moved"""
    cam = tpt.GetSceneDesc()[2].copy()
    cam["origin"][0] += np.float32(0.25)
    return cam


# ---------------------------------------------------------------- the pass
def trace_frame(tpt, w, h, j, flags, time, camera=None):
    """frame j alone (not progressive, zeroed tile and moments plane) -> (its camera record, [colour, albedo, nd, moments] and its
    object plane on the device)"""
    import torch
    if camera is not None:
        tpt.set_camera(**camera)
    flags &= ~FLAG_PROGRESSIVE
    tpt.UpdateTest(time, j, w, h, flags)
    cam = tpt.GetSceneDesc()[2].copy()
    tile, mo, alb, nd = plane(h, w), plane(h, w), plane(h, w, float("nan")), plane(h, w, float("nan"))
    torch.cuda.synchronize()
    tpt.draw_device_moments(time, j, w, h, tile.data_ptr(), mo.data_ptr(), flags, albedo_ptr=alb.data_ptr(), normal_depth_ptr=nd.data_ptr())
    obj = object_planes(tpt, w, h)[0]
    return cam, [tile, alb, nd, mo], obj


def accumulate(tpt, w, h, cam, cur, obj, prev, motion=None, **kw):
    """the pass on device planes -> its four outputs on the device.  prev: None or (camera, colour, albedo, nd, moments, object);
    motion: None or a device tensor [n, 4]"""
    import torch
    outs = [plane(h, w, float("nan")) for _ in range(4)]
    torch.cuda.synchronize()
    tpt.temporal_accumulate_objects_device(w, h, cam, *[t.data_ptr() for t in cur], obj.data_ptr(), *[t.data_ptr() for t in outs],
                                           prev=None if prev is None else (prev[0],) + tuple(t.data_ptr() for t in prev[1:]),
                                           motion_ptr=None if motion is None else motion.data_ptr(),
                                           n_objects=0 if motion is None else motion.shape[0], **kw)
    return outs


def run_chain(tpt, checker, w, h, frames, flags=0, time=lambda j: 0.0, camera=lambda j: None, table=lambda j: None, **kw):
    """`frames` frames chained through the pass; every frame's object plane and outputs equal the checker's on the GPU's own previous
    outputs, and no input is written.  -> (the history lengths, the object plane) of the last frame"""
    prev = None
    N = ids = None
    for j in range(frames):
        cam, cur, obj = trace_frame(tpt, w, h, j, flags, time(j), camera(j))
        motion = table(j)
        dmotion = None if motion is None else dev(motion)
        tpt.synchronize()
        ins = cur + [obj] + ([] if prev is None else list(prev[1:])) + ([] if dmotion is None else [dmotion])
        before = host(ins)
        ids = before[4]
        assert ids.tobytes() == checker.plane(tpt.GetSceneDesc()[0], cam, w, h)[0].tobytes(), "frame %d: the object plane" % j
        outs = accumulate(tpt, w, h, cam, cur, obj, prev, dmotion, **kw)
        tpt.synchronize()
        got = host(outs)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, host(ins))), "frame %d: an input was written" % j
        hprev = None if prev is None else (prev[0],) + tuple(before[5:10])
        want = checker.run(cam, tuple(before[:4]), ids, hprev, motion, **kw)
        for name, g, wnt in zip(NAMES, got, want):
            assert g.tobytes() == wnt.tobytes(), "frame %d: out %s differs from the checker" % (j, name)
        N = got[2][..., 3]
        assert (got[3][..., 0] == 0).all() and (got[3][..., 1] >= 0).all() and (N >= 1).all()
        prev = (cam, outs[0], outs[1], cur[2], outs[2], obj)
    return N, ids


def test_animated_scene_chain_with_the_motion_table(tpt_defaults, checker):
    tpt = tpt_defaults
    step = 0.3  # (spheres 1 and 8 move by several pixels per frame)
    table = lambda j: None if j == 0 else tpt.object_motion_table(step * j, step * (j - 1), FLAG_ANIMATE)  # noqa: E731
    N, ids = run_chain(tpt, checker, 256, 144, 5, flags=FLAG_ANIMATE, time=lambda j: step * j, table=table)
    assert (N == 4).mean() > 0.7
    moving = np.isin(ids, (1, 8))
    assert moving.sum() > 200 and (N[moving] > 1).mean() > 0.5  # the moving spheres carry history


def test_orbiting_camera_chain_with_capped_mirrors_and_glass(tpt_defaults, checker):
    tpt = tpt_defaults
    spheres, mats = tpt.GetSceneDesc()[:2]
    caps = np.where(mats["type"] != 0, 2.0, 0.0).astype(np.float32)
    table = tpt.motion_table(spheres, spheres, caps)
    assert (table[:, :3] == 0).all() and (caps == 2).sum() > 10
    N, ids = run_chain(tpt, checker, 256, 144, 5, camera=lambda j: orbit(j, 0.5), table=lambda j: table, max_history=8.0)
    capped = np.isin(ids, np.nonzero(caps)[0])
    assert capped.sum() > 500 and (N[capped] <= 2).all() and (N[capped] == 2).any()
    assert (N[~capped] > 2).mean() > 0.5


def test_grouped_scene_chain_without_a_table(tpt_defaults, checker):
    from toypathtracer_amd.scenes import stress_scene
    tpt = tpt_defaults
    s, m = stress_scene(4096, 64)
    tpt.set_scene(s, m)
    step = lambda j: dict(look_from=(0.05 * j, 6.0, 20.0), look_at=(0.0, 0.0, 0.0), vfov=60.0, aperture=0.02, focus_dist=20.0)  # noqa: E731
    N, _ = run_chain(tpt, checker, 192, 108, 3, camera=step, max_history=16.0, coverage_tolerance=0.25)
    assert tpt.scene_info()["groups"] > 0 and (N > 1).mean() > 0.3


def camera_record(c):
    from toypathtracer_amd.api import CAMERA_DT
    return np.frombuffer(c.tobytes(), CAMERA_DT)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_synthetic_planes(tpt_defaults, checker, kind, size):
    tpt = tpt_defaults
    w, h = size
    cam, cur, obj, prev, motion = synthetic_objects(kind, w, h)
    kw = dict(max_history=8.0, depth_tolerance=0.1, normal_tolerance=0.25, coverage_tolerance=0.0)
    dcur, dobj, dmotion = [dev(a) for a in cur], dev(obj), dev(motion)
    dprev = None if prev is None else (camera_record(prev[0]),) + tuple(dev(a) for a in prev[1:])
    for table, dtable in ((motion, dmotion), (None, None)):
        outs = accumulate(tpt, w, h, camera_record(cam), dcur, dobj, dprev, dtable, **kw)
        tpt.synchronize()
        want = checker.run(cam, cur, obj, prev, table, **kw)
        for name, g, wnt in zip(NAMES, host(outs), want):
            assert g.tobytes() == wnt.tobytes(), "out %s differs from the checker (table %s)" % (name, table is not None)
    for a, d in zip(list(cur) + [obj, motion] + (list(prev[1:]) if prev else []), dcur + [dobj, dmotion] + (list(dprev[1:]) if dprev else [])):
        assert a.tobytes() == d.cpu().numpy().tobytes(), "an input was written"


def test_no_table_and_one_id_is_the_plain_entry_point(tpt_defaults):
    import torch
    tpt = tpt_defaults
    w, h = 256, 144
    frames = []
    for j in range(2):
        cam, cur, _ = trace_frame(tpt, w, h, j, 0, 0.0, orbit(j, 0.5))
        frames.append((cam, cur))
    (pcam, pcur), (cam, cur) = frames
    pcur[3][..., 3] = 1.0  # (a previous frame's moments carry a history length)
    torch.cuda.synchronize()
    plain = [plane(h, w, float("nan")) for _ in range(4)]
    tpt.temporal_accumulate_device(w, h, cam, *[t.data_ptr() for t in cur], *[t.data_ptr() for t in plain],
                                   prev=(pcam,) + tuple(t.data_ptr() for t in pcur))
    tpt.synchronize()
    plain = host(plain)
    assert (plain[2][..., 3] > 1).mean() > 0.5
    for const in (-1, 0, 45):
        ids = torch.full((h, w), const, dtype=torch.int32, device="cuda")
        outs = accumulate(tpt, w, h, cam, cur, ids, (pcam,) + tuple(pcur) + (ids,))
        tpt.synchronize()
        assert all(g.tobytes() == p.tobytes() for g, p in zip(host(outs), plain)), const


def test_a_sphere_moved_with_set_scene_keeps_its_history(tpt_defaults, checker):
    """Two frames of a 9-sphere scene at 160x90 in which tptSetScene moves sphere 5 sideways by its radius: more pixels of that sphere
    reach N == 2 through the pass with api.motion_table than through tptTemporalAccumulateDevice on the same planes, which finds the
    sphere's old surface (another normal) or what stood behind it; and every output equals the checker's, whose taps are of one id."""
    import torch
    tpt = tpt_defaults
    w, h, which = 160, 90, 5
    spheres, mats = tpt.GetSceneDesc()[:2]
    s0, m0 = spheres[:9].copy(), mats[:9].copy()
    s1 = s0.copy()
    s1["cx"][which] += s0["radius"][which]
    tpt.set_scene(s0, m0)
    pcam, pcur, pobj = trace_frame(tpt, w, h, 0, 0, 0.0)
    tpt.set_scene(s1, m0)
    cam, cur, obj = trace_frame(tpt, w, h, 1, 0, 0.0)
    pcur[3][..., 3] = 1.0
    table = tpt.motion_table(s0, s1)
    assert table[which].tolist() == [-0.5, 0, 0, 0] and np.count_nonzero(table) == 1
    dtable = dev(table)
    prev = (pcam,) + tuple(pcur) + (pobj,)
    outs = accumulate(tpt, w, h, cam, cur, obj, prev, dtable)
    plain = [plane(h, w, float("nan")) for _ in range(4)]
    torch.cuda.synchronize()
    tpt.temporal_accumulate_device(w, h, cam, *[t.data_ptr() for t in cur], *[t.data_ptr() for t in plain],
                                   prev=(pcam,) + tuple(t.data_ptr() for t in pcur))
    tpt.synchronize()
    ids = obj.cpu().numpy()
    on = ids == which
    n_new = int((outs[2].cpu().numpy()[..., 3][on] == 2).sum())
    n_plain = int((plain[2].cpu().numpy()[..., 3][on] == 2).sum())
    print("sphere %d covers %d pixels; N == 2 on it: followed %d, plain pass %d" % (which, int(on.sum()), n_new, n_plain))
    assert on.sum() > 200 and n_new > n_plain
    want = checker.run(cam, tuple(host(cur)), ids, (pcam,) + tuple(host(pcur)) + (pobj.cpu().numpy(),), table)
    for name, g, wnt in zip(NAMES, host(outs), want):
        assert g.tobytes() == wnt.tobytes(), "out %s differs from the checker" % name


def test_refusals_leave_out_untouched(tpt_defaults):
    import torch
    tpt = tpt_defaults
    lib = tpt.load_library()
    w, h = 64, 40
    cam, cur, prev = synthetic_case("same", w, h)
    cams = [C.create_string_buffer(c.tobytes(), 88) for c in (cam, prev[0])]
    ins = [dev(a) for a in cur] + [dev(a) for a in prev[1:]]
    outs = [plane(h, w, float("nan")) for _ in range(4)]
    big = plane(2 * h, w, float("nan"))
    ids = [torch.full((h, w), k, dtype=torch.int32, device="cuda") for k in (3, 3)]
    motion = torch.zeros((5, 4), dtype=torch.float32, device="cuda")
    planes = torch.full((2, h, w), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    count = [0]

    def untouched(what):
        tpt.synchronize()
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in outs + [big]) and bool((planes == -9).all()), "a refused call wrote an output: " + what
        count[0] += 1

    def refused(what, ww=w, hh=h, pc=1, i=None, o=None, mh=4.0, ob=ids[0].data_ptr(), pob=ids[1].data_ptr(), m=motion.data_ptr(), n=5):
        ptrs = [t.data_ptr() for t in ins + outs]
        for k, v in list((i or {}).items()) + [(8 + k, v) for k, v in (o or {}).items()]:
            ptrs[k] = v
        vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        rc = lib.tptTemporalAccumulateObjectsDevice(ww, hh, cams[0], None if pc is None else cams[pc], *[vp(p) for p in ptrs], C.c_float(mh),
                                                    C.c_float(0.1), C.c_float(0.25), C.c_float(0.0), vp(ob), vp(pob), vp(m), n)
        msg = lib.tptGetLastError().decode()
        assert rc != 0 and "tptTemporalAccumulateObjectsDevice" in msg, (what, msg)
        untouched(what)

    refused("w 0", ww=0)
    refused("output 2 NULL", o={2: 0})
    refused("prevCamera alone NULL", pc=None)
    refused("an output is an input", o={0: ins[1].data_ptr()})
    refused("maxHistory 0.5", mh=0.5)
    refused("object NULL", ob=0)
    refused("prevObject NULL with the prev planes", pob=0)
    refused("prevObject on the first frame", pc=None, i={4: 0, 5: 0, 6: 0, 7: 0})
    refused("nObjects -1", n=-1)
    refused("nObjects 65535", n=65535)
    refused("a table without a count", n=0)
    refused("a count without a table", m=0)
    refused("an output is the object plane", o={0: big.data_ptr()}, ob=big.data_ptr() + 16 * w * h - 4)
    refused("an output overlaps the previous object plane", o={1: big.data_ptr() + 4 * w * h - 4}, pob=big.data_ptr())
    refused("an output holds the table", o={3: big.data_ptr()}, m=big.data_ptr() + 64, n=1)

    def plane_refused(what, n=1, ww=w, hh=h, out=planes.data_ptr(), cameras=None, flags=0):
        rc = lib.tptObjectPlaneDevice(n, None, cameras, ww, hh, C.c_void_p(out) if out else None, flags)
        msg = lib.tptGetLastError().decode()
        assert rc != 0 and "tptObjectPlaneDevice" in msg, (what, msg)
        untouched(what)

    tpt.UpdateTest(0.0, 0, w, h, 0)
    plane_refused("nFrames 0", n=0)
    plane_refused("nFrames 4097", n=4097)
    plane_refused("w 8193", ww=8193, cameras=cams[0])
    plane_refused("output NULL", out=0)
    plane_refused("another size without cameras", hh=h + 1)
    plane_refused("a camera that is not finite", cameras=C.create_string_buffer(np.full(22, np.nan, np.float32).tobytes(), 88))
    plane_refused("flags 4", flags=4)
    assert count[0] == 15 + 7
