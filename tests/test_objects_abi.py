"""tptObjectPlaneDevice, tptObjectMotionTable and tptTemporalAccumulateObjectsDevice without a GPU: the declarations, bindings and
exports; the bindings' argument checks; the gfx950 code of the new kernels in the shipped library; and the refusals and the motion
table, driven through the host runtime compiled against tests/hostemu (a refused call returns before anything is enqueued; the
launchers are tests/hostemu_objects.cpp, which count and run nothing, and show what the host made of cameras, times and scene)."""
import re

import numpy as np
import pytest

from isa_lib import code_object, count, exported_symbols, header_params, no_library, refusal_messages, refused_without_its_launcher, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import OBJECT_PLANE as PLANE, REPROJECT, TEMPORAL, family

TEMPORAL_PARAMS = [
    "int screenWidth", "int screenHeight", "const void* camera", "const void* prevCamera", "const float* deviceColour",
    "const float* deviceAlbedo", "const float* deviceNormalDepth", "const float* deviceMoments", "const float* devicePrevColour",
    "const float* devicePrevAlbedo", "const float* devicePrevNormalDepth", "const float* devicePrevMoments", "float* deviceOutColour",
    "float* deviceOutAlbedo", "float* deviceOutMoments", "float* deviceOutVariance", "float maxHistory", "float depthTolerance",
    "float normalTolerance", "float coverageTolerance"]
NEW = ("tptObjectPlaneDevice", "tptObjectMotionTable", "tptTemporalAccumulateObjectsDevice")


def test_header_declares_the_entry_points():
    assert header_params("tptObjectPlaneDevice") == [
        "int nFrames", "const float* times", "const void* cameras", "int screenWidth", "int screenHeight", "int32_t* deviceFrameObjects",
        "unsigned testFlags"]
    assert header_params("tptObjectMotionTable") == ["float time", "float prevTime", "unsigned testFlags", "float* outTable", "int capacity"]
    assert header_params("tptTemporalAccumulateDevice") == TEMPORAL_PARAMS
    assert header_params("tptTemporalAccumulateObjectsDevice") == TEMPORAL_PARAMS + [
        "const int32_t* deviceObject", "const int32_t* devicePrevObject", "const float* deviceObjectMotion", "int nObjects"]


def test_bindings_and_exports():
    from toypathtracer_amd import api
    lib = api.load_library()
    out = exported_symbols(api.library_path())
    for name in NEW:
        assert name in api.C_ABI_SYMBOLS and hasattr(lib, name)
        assert re.search(r"\bT %s\b" % name, out), name
    for fn in (api.object_plane_device, api.object_motion_table, api.motion_table, api.temporal_accumulate_objects_device):
        assert callable(fn)


def camera(n=1):
    from toypathtracer_amd import api
    return np.zeros(n, api.CAMERA_DT)


@pytest.mark.parametrize("args", [
    dict(w=0), dict(h=-3), dict(w=8.0), dict(h=True), dict(objects_ptr=0), dict(objects_ptr=None), dict(objects_ptr=1.5), dict(flags=4),
    dict(flags=-1), dict(flags=1.0), dict(times=[[0.0]]), dict(times=[0.0, 1.0], frames=3), dict(cameras=np.zeros(22, np.float32)),
    dict(cameras="x"), dict(cameras=np.zeros((2, 1), [("a", "<f4", 22)])), dict(times=[0.0], cameras=2), dict(frames=0), dict(frames=4097),
    dict(frames=2.0), dict(times=[]), dict(times=[0.0] * 4097),
], ids=lambda a: ",".join("%s=%.20r" % kv for kv in a.items()))
def test_object_plane_binding_checks_arguments_before_the_library(monkeypatch, args):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(w=16, h=8, objects_ptr=4096, flags=0, times=None, cameras=None, frames=None)
    a.update(args)
    if isinstance(a["cameras"], int):
        a["cameras"] = camera(a["cameras"])
    with pytest.raises(ValueError):
        api.object_plane_device(a["w"], a["h"], a["objects_ptr"], a["flags"], times=a["times"], cameras=a["cameras"], frames=a["frames"])


@pytest.mark.parametrize("args", [
    dict(w=0), dict(h=8.0), dict(camera=None), dict(camera=b"x" * 88), dict(colour=0), dict(nd=1.5), dict(object=0), dict(object=None),
    dict(object=-4), dict(out_variance=0), dict(prev=()), dict(prev="camera"), dict(prev5=True), dict(prev_object=0),
    dict(prev_object=None), dict(prev_object=2.0), dict(motion_ptr=4096), dict(n_objects=3), dict(motion_ptr=4096, n_objects=-1),
    dict(motion_ptr=4096, n_objects=65535), dict(motion_ptr=4096, n_objects=2.0), dict(motion_ptr=-1, n_objects=1),
    dict(motion_ptr="m", n_objects=1), dict(max_history=0.5), dict(max_history=float("nan")), dict(depth_tolerance=-0.1),
    dict(normal_tolerance=float("inf")), dict(coverage_tolerance=float("nan")),
], ids=lambda a: ",".join("%s=%.20r" % kv for kv in a.items()))
def test_pass_binding_checks_arguments_before_the_library(monkeypatch, args):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(w=16, h=8, camera=camera(), colour=4096, albedo=8192, nd=12288, mo=16384, object=53248, out_colour=20480, out_albedo=24576,
             out_moments=28672, out_variance=32768, prev=(camera(), 36864, 40960, 45056, 49152, 57344), motion_ptr=None, n_objects=0)
    if "prev_object" in args:
        a["prev"] = a["prev"][:5] + (args.pop("prev_object"),)
    if args.pop("prev5", False):
        a["prev"] = a["prev"][:5]  # (tptTemporalAccumulateDevice's five: the object plane is missing)
    a.update(args)
    kw = {k: a.pop(k) for k in list(a) if k in api.TEMPORAL_DEFAULTS}
    with pytest.raises(ValueError):
        api.temporal_accumulate_objects_device(a["w"], a["h"], a["camera"], a["colour"], a["albedo"], a["nd"], a["mo"], a["object"],
                                               a["out_colour"], a["out_albedo"], a["out_moments"], a["out_variance"], prev=a["prev"],
                                               motion_ptr=a["motion_ptr"], n_objects=a["n_objects"], **kw)


def test_motion_table_helpers(monkeypatch):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    for bad in (dict(time="0"), dict(prev_time=None), dict(time=True), dict(flags=-1), dict(flags=1.5)):
        a = dict(time=0.0, prev_time=1.0, flags=1)
        a.update(bad)
        with pytest.raises(ValueError):
            api.object_motion_table(a["time"], a["prev_time"], a["flags"])
    cur = np.zeros(3, api.SPHERE_DT)
    prev = cur.copy()
    cur["cx"], prev["cx"] = [1, 2, 3], [1, 2.5, 3]
    cur["cz"], prev["cz"] = [0.1, 0, 0], [0.3, 0, 0]
    t = api.motion_table(prev, cur)
    assert t.dtype == np.float32 and t.shape == (3, 4)
    want = np.zeros((3, 4), np.float32)
    want[1, 0] = 0.5
    want[0, 2] = np.float32(0.3) - np.float32(0.1)
    assert t.tobytes() == want.tobytes()
    assert (api.motion_table(prev, cur, caps=2)[:, 3] == 2).all()
    assert api.motion_table(prev, cur, caps=[0, 1, 2.5])[:, 3].tolist() == [0, 1, 2.5]
    for bad in (dict(caps=[1, 2]), dict(caps=-1), dict(caps=[[1, 2, 3]]), dict(prev=prev[:2]), dict(prev=np.zeros((3, 5), np.float32)),
                dict(cur=None)):
        a = dict(prev=prev, cur=cur, caps=None)
        a.update(bad)
        with pytest.raises(ValueError):
            api.motion_table(a["prev"], a["cur"], a["caps"])


def test_exactly_the_new_kernels_are_in_the_code_object(code_object):  # noqa: F811
    """(every other family, the plain pass's among them: tests/test_isa_contract.py holds the library to exactly
    tests/kernel_manifest.py)"""
    _, meta = code_object
    assert sorted(n for n in meta if "Object" in n) == sorted([PLANE] + family(REPROJECT))


@pytest.mark.parametrize("history", [1, 0], ids=["history", "first-frame"])
def test_reproject_kernels_in_the_code_object(code_object, history):  # noqa: F811
    bodies, meta = code_object
    name = REPROJECT % history
    assert name in meta and name in bodies, "the object-following kernel is missing from the shipped code object"
    body, m = bodies[name], meta[name]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert count(body, r"scratch_") == 0
    assert count(body, r"flat_") == 0, "a FLAT instruction: a global pointer lost its address space"
    assert count(body, r"ds_") == 0 and m["group_segment_fixed_size"] == 0 and m["agpr_count"] == 0
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64
    assert m["vgpr_count"] <= 64, m  # (eight waves per SIMD: the plain kernel's ceiling)
    assert count(body, r"global_store_dwordx4") == 4 and count(body, r"global_store") == 4
    assert count(body, r"global_atomic|buffer_") == 0
    loads, plain = count(body, r"global_load"), count(bodies[TEMPORAL % history], r"global_load")
    if history:
        assert loads > plain  # the id planes and the table on top of the plain pass's loads
    else:
        assert loads <= 4, "the first-frame form reads more than this frame's planes"
        assert count(body, r"v_sqrt|v_rsq") == 0  # (and projects nothing)


def test_object_plane_kernel_in_the_code_object(code_object):  # noqa: F811
    bodies, meta = code_object
    assert PLANE in meta and PLANE in bodies, "the object-plane kernel is missing from the shipped code object"
    body, m = bodies[PLANE], meta[PLANE]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert count(body, r"scratch_") == 0
    assert count(body, r"flat_") == 0, "a FLAT instruction: a pointer lost its address space"
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64 and m["agpr_count"] == 0
    assert count(body, r"global_store_dword$") == 1 and count(body, r"global_store") == 1  # one id per pixel
    assert count(body, r"global_atomic|buffer_") == 0
    # the sphere records are wave-uniform: scalar loads through the constant address space, no vector load and no LDS
    assert count(body, r"global_load") == 0 and count(body, r"ds_") == 0 and m["group_segment_fixed_size"] == 0
    assert count(body, r"s_load_dwordx4") >= 1
    assert m["vgpr_count"] <= 32, m


REFUSALS = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from toypathtracer_amd import api as tpt
from temporal_lib import look_at_camera
from oracle_lib import Oracle
lib = tpt.load_library()
oracle = Oracle.get()
w, h = 16, 8
ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
def msg(): return lib.tptGetLastError().decode()
# ---------------------------------------------------------------- the motion table
def table(t, pt, flags, cap=None, out="own"):
    n = tpt.GetObjectCount()[0]
    buf = np.full((n + 2, 4), np.nan, np.float32)
    rc = lib.tptObjectMotionTable(t, pt, flags, None if out is None else buf.ctypes.data, n if cap is None else cap)
    return rc, buf
rc, _ = table(0.0, 1.0, 1)
assert rc != 0 and "not initialised" in msg(), msg()
print("refused: table, no context --", msg())
tpt.InitializeTest()
so = C.CDLL(tpt.library_path())
for what, kw in (("outTable NULL", dict(out=None)), ("capacity 45", dict(cap=45)), ("capacity 0", dict(cap=0)), ("capacity -1", dict(cap=-1))):
    rc, buf = table(0.5, 0.25, 1, **kw)
    assert rc != 0 and "tptObjectMotionTable" in msg() and np.isnan(buf).all(), (what, rc, msg())
    print("refused: table,", what, "--", msg())
spheres0, mats0 = tpt.GetSceneDesc()[:2]
def expect(t, pt):
    a, b = spheres0.copy(), spheres0.copy()
    oracle.lib.tpto_animate(a.ctypes.data, C.c_float(t)); oracle.lib.tpto_animate(b.ctypes.data, C.c_float(pt))
    want = np.zeros((46, 4), np.float32)
    want[1, 1] = b["cy"][1] - a["cy"][1]
    want[8, 2] = b["cz"][8] - a["cz"][8]
    return want
for t, pt in ((0.5, 0.25), (0.0, 0.0), (3.0, -7.5), (1e6, 0.1)):
    rc, buf = table(t, pt, 1)
    assert rc == 0, msg()
    want = expect(t, pt)
    assert buf[:46].tobytes() == want.tobytes() and np.isnan(buf[46:]).all(), (t, pt, buf[[1, 8]], want[[1, 8]])
    assert (t == pt) or (want[1, 1] != 0 and want[8, 2] != 0)
    assert tpt.object_motion_table(t, pt, 1).tobytes() == want.tobytes()
    rc, buf = table(t, pt, 3, cap=1000)
    assert rc == 0 and buf[:46].tobytes() == want.tobytes()
    for flags in (0, 2):
        rc, buf = table(t, pt, flags)
        assert rc == 0 and (buf[:46] == 0).all() and not np.signbit(buf[:46]).any() and np.isnan(buf[46:]).all()
rc, buf = table(float("nan"), 0.0, 1)
assert rc == 0 and np.isnan(buf[1, 1]) and np.isnan(buf[8, 2]) and np.isfinite(np.delete(buf[:46].ravel(), [5, 34])).all()
print("accepted: the built-in scene's table")
tpt.set_scene(spheres0[:8], mats0[:8])
rc, buf = table(0.5, 0.25, 1)
assert rc == 0 and (buf[:8] == 0).all() and np.isnan(buf[8:]).all()
print("accepted: 8 spheres, all zero")
tpt.set_scene(spheres0[:9], mats0[:9])
rc, buf = table(0.5, 0.25, 1)
assert rc == 0 and buf[:9].tobytes() == expect(0.5, 0.25)[:9].tobytes() and np.isnan(buf[9:]).all()
print("accepted: 9 spheres")
tpt.set_scene(None, None)
assert tpt.GetSceneDesc()[0].tobytes() == spheres0.tobytes(), "the table moved the scene"
# ---------------------------------------------------------------- the object plane
P = "tptObjectPlaneDevice"
cam = look_at_camera([0.0, 2.0, 3.0], [0.0, 0.0, 0.0], w, h)
cams = np.stack([cam, look_at_camera([0.5, 2.0, 3.0], [0.0, 0.0, 0.0], w, h), look_at_camera([1.0, 2.0, 3.0], [0.0, 0.0, 0.0], w, h)])
planes = np.full((3, h, w), -7, np.int32)
times = np.array([0.25, 0.5, np.nan], np.float32)
def plane(n=1, t=None, c=cams, ww=w, hh=h, out=planes, flags=0):
    return lib.tptObjectPlaneDevice(n, ptr(t), ptr(c), ww, hh, ptr(out), flags)
def refused(what, fn, expect, **kw):
    rc = fn(**kw)
    assert rc != 0 and expect in msg(), (what, rc, msg())
    print("refused:", what, "--", msg())
refused("plane: before any tptUpdate", plane, P)
tpt.UpdateTest(0.0, 0, w, h, 0)
for n in (0, -1, 4097):
    refused("plane: nFrames %d" % n, plane, P, n=n, c=None)
for ww, hh in ((0, h), (w, 0), (8193, 1), (1, 8193), (-4, -4)):
    refused("plane: size %dx%d" % (ww, hh), plane, P, ww=ww, hh=hh)
refused("plane: output NULL", plane, P, out=None)
refused("plane: cameras NULL at another size", plane, P, c=None, hh=h + 1)
refused("plane: cameras NULL at another width", plane, P, c=None, ww=w + 1)
for k, v in ((0, np.nan), (4, np.inf), (8, -np.inf), (11, np.nan)):
    bad = cams.copy(); bad[2, k] = v
    refused("plane: camera 2 field %d = %r" % (k, v), plane, P, n=3, c=bad)
for flags in (4, 8, 0x80000000, 7):
    refused("plane: flags %#x" % flags, plane, P, flags=flags)
assert so.hostemuObjectPlaneLaunches() == 0, "a refused call reached the launcher"
so.hostemuObjectPlaneConsts.restype = C.POINTER(C.c_float * 18)
so.hostemuObjectPlaneConsts.argtypes = [C.c_int]
so.hostemuObjectPlaneOut.restype = C.c_void_p
def launch(k): return np.array(so.hostemuObjectPlaneConsts(k).contents, np.float32)
scene_before = [a.tobytes() for a in tpt.GetSceneDesc()[:3]]
# accepted: the update's camera; a field beyond the first twelve may be anything
own = tpt.GetSceneDesc()[2].view(np.float32).reshape(22)
assert plane(c=None) == 0, msg()
k = launch(0)
assert k[:12].tobytes() == own[:12].tobytes() and so.hostemuObjectPlaneSpheres(0) == 46
s1, s8 = spheres0[1], spheres0[8]
assert k[12:].tolist() == [s1["cx"], s1["cy"], s1["cz"], s8["cx"], s8["cy"], s8["cz"]]
print("accepted: the update's camera")
odd = cams.copy(); odd[:, 12:] = np.nan
assert plane(n=3, t=times, c=odd, flags=1) == 0, msg()
assert so.hostemuObjectPlaneLaunches() == 4
for j in range(3):
    k = launch(1 + j)
    assert k[:12].tobytes() == cams[j, :12].tobytes(), j
    moved = spheres0.copy()
    oracle.lib.tpto_animate(moved.ctypes.data, C.c_float(times[j]))
    want = np.array([s1["cx"], moved["cy"][1], s1["cz"], s8["cx"], s8["cy"], moved["cz"][8]], np.float32)
    assert k[12:].tobytes() == want.tobytes(), (j, k[12:], want)  # (a NaN time: its own frame's centres alone)
    assert so.hostemuObjectPlaneOut(1 + j) == planes.ctypes.data + 4 * w * h * j
print("accepted: three frames, cameras and times")
for what, kw in (("no flag", dict(t=times, flags=2)), ("no times", dict(flags=1)), ("both flags, no times", dict(flags=3))):
    before = so.hostemuObjectPlaneLaunches()
    assert plane(n=3, **kw) == 0, msg()
    for j in range(3):
        assert launch(before + j)[12:].tolist() == [s1["cx"], s1["cy"], s1["cz"], s8["cx"], s8["cy"], s8["cz"]], (what, j)
    print("accepted:", what)
assert plane(n=1, ww=8192, hh=1, out=np.zeros(8192, np.int32)) == 0, msg()
print("accepted: 8192 x 1")
assert [a.tobytes() for a in tpt.GetSceneDesc()[:3]] == scene_before, "the object plane changed the context's scene or camera"
# the scene as of the last update: 8 spheres do not move, 9 do; a later tptSetScene plays no part
for count, moves in ((8, False), (9, True)):
    tpt.set_scene(spheres0[:count], mats0[:count])
    tpt.UpdateTest(0.0, 0, w, h, 0)
    tpt.set_scene(None, None)
    before = so.hostemuObjectPlaneLaunches()
    assert plane(n=1, t=times[1:], flags=1) == 0, msg()
    k = launch(before)
    assert so.hostemuObjectPlaneSpheres(before) == count
    assert (k[13] != s1["cy"]) == moves and (count < 9 or (k[17] != s8["cz"])), (count, k[12:])
    print("accepted: %d spheres" % count)
tpt.UpdateTest(0.0, 0, w, h, 0)
tpt.synchronize()
assert (planes == -7).all(), "a call wrote an output (the stand-in runs nothing)"
# ---------------------------------------------------------------- the pass
T = "tptTemporalAccumulateObjectsDevice"
pcam = cams[1]
ins = [np.full((h, w, 4), 0.25 + k, np.float32) for k in range(8)]
outs = [np.full((h, w, 4), np.nan, np.float32) for k in range(4)]
big = np.full((2 * h, w, 4), np.nan, np.float32)
obj, pobj = np.full((h, w), 3, np.int32), np.full((h, w), 4, np.int32)
motion = np.full((5, 4), 0.5, np.float32)
def call(ww=w, hh=h, c=cam, pc=pcam, i={}, o={}, mh=4.0, dt=0.1, nt=0.25, ct=0.0, ob=obj, pob=pobj, m=motion, n=5):
    pl = list(ins) + list(outs)
    for k, v in i.items(): pl[k] = v
    for k, v in o.items(): pl[8 + k] = v
    return lib.tptTemporalAccumulateObjectsDevice(ww, hh, ptr(c), ptr(pc), *[ptr(p) for p in pl], mh, dt, nt, ct, ptr(ob), ptr(pob), ptr(m), n)
def changed(c, k, v):
    c = c.copy(); c[k] = v; return c
first = dict(pc=None, i={4: None, 5: None, 6: None, 7: None}, pob=None)
# what the plain pass refuses
for ww, hh in ((0, h), (w, 0), (8193, 1), (1, 8193)):
    refused("pass: size %dx%d" % (ww, hh), call, T, ww=ww, hh=hh)
refused("pass: camera NULL", call, T, c=None)
for k in range(4):
    refused("pass: current plane %d NULL" % k, call, T, i={k: None})
    refused("pass: output %d NULL" % k, call, T, o={k: None})
refused("pass: prevCamera alone NULL", call, T, pc=None)
for k in range(4, 8):
    refused("pass: prev plane %d alone NULL" % k, call, T, i={k: None})
refused("pass: prevCamera alone given", call, T, i={4: None, 5: None, 6: None, 7: None})
for k in range(8):
    refused("pass: output %d is input %d" % (k % 4, k), call, T, o={k % 4: ins[k]})
refused("pass: two outputs are one", call, T, o={0: outs[1]})
for mh in (0.0, 0.999, 65536.5, float("nan")):
    refused("pass: maxHistory %r" % mh, call, T, mh=mh)
for name in ("dt", "nt", "ct"):
    for v in (-1e-6, float("nan"), float("inf")):
        refused("pass: %s %r" % (name, v), call, T, **{name: v})
for which, base in (("c", cam), ("pc", pcam)):
    refused("pass: %s field 5 = inf" % which, call, T, **{which: changed(base, 5, np.inf)})
    flat = base.copy(); flat[6:9] = 0
    refused("pass: %s: dot(H, H) == 0" % which, call, T, **{which: flat})
# and its own
refused("pass: object NULL", call, T, ob=None)
refused("pass: prevObject NULL with the prev planes", call, T, pob=None)
refused("pass: prevObject given on the first frame", call, T, **dict(first, pob=pobj))
for n in (-1, 65535, 1 << 30):
    refused("pass: nObjects %d" % n, call, T, n=n)
refused("pass: a table without a count", call, T, n=0)
refused("pass: a count without a table", call, T, m=None, n=5)
plane_b, words = w * h * 16, w * h * 4
refused("pass: an output is the object plane", call, T, o={0: big}, ob=big.ctypes.data)
refused("pass: an output's tail holds the object plane's head", call, T, o={1: big}, ob=big.ctypes.data + plane_b - 4)
refused("pass: the object plane's tail holds an output's head", call, T, o={2: big.ctypes.data + words - 4}, ob=big)
refused("pass: an output overlaps the previous object plane", call, T, o={3: big}, pob=big.ctypes.data + 64)
refused("pass: an output holds the table", call, T, o={0: big}, m=big.ctypes.data + plane_b - 16, n=1)
refused("pass: the table's last entry lies in an output", call, T, o={1: big.ctypes.data + 4 * 16}, m=big, n=5)
# two rules broken at once: the one that is checked first is the one reported
def order(expect, **kw):
    rc = call(**kw)
    assert rc != 0 and msg() == T + ": " + expect, (expect, sorted(kw), rc, msg())
    print("order:", sorted(kw), "--", expect)
order("two outputs overlap", o={0: outs[1]}, ob=None)  # (the plain pass's rules before its own)
order("maxHistory must lie in 1..65536", mh=0.0, ob=None)
order("deviceObject is required", ob=None, pob=None)
order("devicePrevObject must be given exactly when prevCamera and the prev planes are", pob=None, n=-1)
order("nObjects must lie in 0..65534", n=65535, m=None)
order("deviceObjectMotion and nObjects must be given together", n=0, o={0: big}, ob=big.ctypes.data)
assert so.hostemuObjectPassLaunches() == 0, "a refused call reached the launcher"
so.hostemuObjectPassConsts.restype = C.POINTER(C.c_float * 34)
accepted = (dict(), first, dict(m=None, n=0), dict(first, m=None, n=0), dict(n=1), dict(n=65534, m=np.zeros((65534, 4), np.float32)),
            dict(o={0: big}, ob=big.ctypes.data + plane_b), dict(o={0: big.ctypes.data + words}, ob=big),
            dict(o={1: big.ctypes.data + 5 * 16}, m=big, n=5), dict(ob=obj, pob=obj), dict(pc=cam))
for kw in accepted:
    assert call(**kw) == 0, (sorted(kw), msg())
    print("accepted: pass", sorted(kw))
assert so.hostemuObjectPassLaunches() == len(accepted) and so.hostemuObjectPassObjects() == 5
# the constants are the plain pass's (pc = cam): this camera's fields, a = ll' - o', f = -dot(a, w'), dot(H', H'), dot(V', V')
k = np.array(so.hostemuObjectPassConsts().contents, np.float32)
a = cam[3:6] - cam[0:3]
dot = lambda u, v: np.float32(np.float32(u[0] * v[0] + u[1] * v[1]) + u[2] * v[2])
want = np.concatenate([cam[0:12], cam[0:3], a, cam[18:21], cam[6:12], [-dot(a, cam[18:21]), dot(cam[6:9], cam[6:9]), dot(cam[9:12], cam[9:12])],
                       [4.0, 0.1, 0.25, 0.0]]).astype(np.float32)
assert k.tobytes() == want.tobytes(), (k, want)
tpt.synchronize()
assert all(np.isnan(o).all() for o in outs) and np.isnan(big).all(), "a refused call wrote an output"
assert all((p == 0.25 + n).all() for n, p in enumerate(ins)) and (obj == 3).all() and (pobj == 4).all() and (motion == 0.5).all(), "a call wrote an input"
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_and_the_motion_table_through_the_host_runtime():
    out = run_refusals(REFUSALS, "libtpt_hostemu_objects.so", ["hostemu_objects.cpp"])
    table = 1 + 4
    plane = 1 + 3 + 5 + 1 + 2 + 4 + 4
    plain = 4 + 1 + 8 + 1 + 4 + 1 + 8 + 1 + 4 + 9 + 4
    own = 3 + 3 + 2 + 6
    assert out.count("refused:") == table + plane + plain + own, out
    assert out.count("accepted: pass") == 11, out
    assert out.count("order:") == 6, out
    M, P, T = "tptObjectMotionTable: ", "tptObjectPlaneDevice: ", "tptTemporalAccumulateObjectsDevice: "
    assert refusal_messages(out) == {
        "tpt: not initialised (call tptInitialize / InitializeTest first)": 1,
        M + "outTable is required": 1,
        M + "capacity is smaller than the object count": 3,
        P + "call tptUpdate first": 1,
        P + "nFrames must lie in 1..4096": 3,
        P + "w and h must lie in 1..8192": 5,
        P + "deviceFrameObjects is required": 1,
        P + "without cameras the size must be the last tptUpdate's": 2,
        P + "a camera has a non-finite origin, lowerLeftCorner, horizontal or vertical": 4,
        P + "unknown flag bits": 4,
        T + "w and h must lie in 1..8192": 4,
        T + "camera is required": 1,
        T + "the four planes of this frame are required": 4,
        T + "the four output planes are required": 4,
        T + "prevCamera and the four prev planes must be all NULL or all given": 6,
        T + "an output overlaps an input": 8,
        T + "two outputs overlap": 1,
        T + "maxHistory must lie in 1..65536": 4,
        T + "every tolerance must be finite and at least 0": 9,
        T + "camera has a non-finite field, a degenerate frame or its frame behind its origin": 2,
        T + "prevCamera has a non-finite field, a degenerate frame or its frame behind its origin": 2,
        T + "deviceObject is required": 1,
        T + "devicePrevObject must be given exactly when prevCamera and the prev planes are": 2,
        T + "nObjects must lie in 0..65534": 3,
        T + "deviceObjectMotion and nObjects must be given together": 2,
        T + "an output overlaps an object plane or the motion table": 6,
    }


def test_a_build_without_the_launchers_refuses():
    refused_without_its_launcher('''
tpt.UpdateTest(0.0, 0, 16, 8, 0)
objects = np.full((8, 16), -7, np.int32)
rc = lib.tptObjectPlaneDevice(1, None, None, 16, 8, objects.ctypes.data, 0)
tpt.synchronize()
assert (objects == -7).all()
''', "tptObjectPlaneDevice: this build has no object plane kernel")
    refused_without_its_launcher('''
sys.path.insert(0, sys.argv[1] + "/tests")
from temporal_lib import look_at_camera
cam = look_at_camera([0.0, 2.0, 3.0], [0.0, 0.0, 0.0], 16, 8)
ins, outs = [np.full((8, 16, 4), 0.25, np.float32) for _ in range(4)], [np.full((8, 16, 4), np.nan, np.float32) for _ in range(4)]
objects = np.zeros((8, 16), np.int32)
rc = lib.tptTemporalAccumulateObjectsDevice(16, 8, cam.ctypes.data, None, *[p.ctypes.data for p in ins], None, None, None, None,
                                            *[p.ctypes.data for p in outs], 4.0, 0.1, 0.25, 0.0, objects.ctypes.data, None, None, 0)
tpt.synchronize()
assert all(np.isnan(p).all() for p in outs)
''', "tptTemporalAccumulateObjectsDevice: this build has no object-following accumulation kernel")
