"""tptMotionVectorsDevice without a GPU: the declaration, the layout of tptMotionVectorsArgs against the ctypes mirror, the export and
the binding; the binding's argument checks; the gfx950 code of the two new kernels in the shipped library; and the refusals and the
launch plan of accepted calls, driven through the host runtime compiled against tests/hostemu (a refused call returns before anything
is enqueued; the launchers are tests/hostemu_flow.cpp, which shows what the host handed it and what its launch finds in the constants
table when it runs, and tests/hostemu_temporal.cpp, whose constants the table's records are compared with)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from isa_lib import code_object, count, exported_symbols, header, header_params, no_library, refusal_messages, refused_without_its_launcher, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import FLOW, family
from oracle_lib import ROOT

CTYPES_OF = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float}


def struct_fields():
    """tptMotionVectorsArgs as include/tpt_hip.h declares it -> [(name, C type as written)]"""
    body = re.search(r"typedef\s+struct\s+tptMotionVectorsArgs\s*\{(.*?)\}\s*tptMotionVectorsArgs\s*;", header(), flags=re.S)
    assert body, "tptMotionVectorsArgs is not declared in include/tpt_hip.h"
    fields = []
    for decl in body.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(.*?[\s*])(\w+(?:\s*,\s*\w+)*)$", decl)
        ctype = m.group(1).strip()
        fields += [(name.strip(), ctype) for name in m.group(2).split(",")]
    return fields


def test_header_declares_the_entry_point_and_its_struct():
    assert header_params("tptMotionVectorsDevice") == ["const tptMotionVectorsArgs* args"]
    from toypathtracer_amd import api
    fields = struct_fields()
    assert [n for n, _ in fields] == [n for n, _ in api.MotionVectorsArgs._fields_]
    for (name, ctype), (_, mirror) in zip(fields, api.MotionVectorsArgs._fields_):
        assert mirror is (C.c_void_p if ctype.endswith("*") else CTYPES_OF[ctype]), (name, ctype, mirror)
    for name in ("deviceFrameAlbedo", "deviceFrameNormalDepth", "deviceFrameObjectMotion", "devicePrevAlbedo", "devicePrevNormalDepth"):
        assert dict(fields)[name] == "const float*", name  # inputs are never written
    assert dict(fields)["deviceFrameMotion"] == "float*"
    assert dict(fields)["deviceFrameObjects"] == dict(fields)["devicePrevObject"] == "const int32_t*"
    assert dict(fields)["cameras"] == dict(fields)["prevCamera"] == "const void*"
    # the statement is written out in the header, and says what sets it apart from the temporal passes
    text = open(os.path.join(ROOT, "include", "tpt_hip.h")).read()
    doc = text[text.index("A CLIP'S MOTION VECTORS"):text.index("typedef struct tptMotionVectorsArgs")]
    for words in ("TPT_TEMPORAL_SNAP", "PROJECTS", "{0, 0, 0, 0}", "OWN albedo", "history length", "independent", "Refused"):
        assert words in doc, words


def test_struct_layout_matches_the_ctypes_mirror(tmp_path):
    """sizeof and every offsetof, as the C compiler lays the header's struct out"""
    from toypathtracer_amd import api
    names = [n for n, _ in api.MotionVectorsArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tpt_hip.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(tptMotionVectorsArgs));\n'
                   + "".join('    printf("%%zu\\n", offsetof(tptMotionVectorsArgs, %s));\n' % n for n in names) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert got == [C.sizeof(api.MotionVectorsArgs)] + [getattr(api.MotionVectorsArgs, n).offset for n in names]
    assert got[0] == 112


def test_binding_and_export():
    from toypathtracer_amd import api
    name = "tptMotionVectorsDevice"
    assert name in api.C_ABI_SYMBOLS and callable(api.motion_vectors_device)
    lib = api.load_library()
    assert hasattr(lib, name) and lib.tptMotionVectorsDevice.argtypes == [C.POINTER(api.MotionVectorsArgs)]
    assert re.search(r"\bT %s\b" % name, exported_symbols(api.library_path()))
    import inspect
    defaults = {k: v.default for k, v in inspect.signature(api.motion_vectors_device).parameters.items()}
    for k in ("depth_tolerance", "normal_tolerance", "coverage_tolerance"):
        assert defaults[k] == api.TEMPORAL_DEFAULTS[k], k
    assert "max_history" not in defaults


def cameras(n):
    from toypathtracer_amd import api
    return np.zeros(n, api.CAMERA_DT)


@pytest.mark.parametrize("args", [
    dict(w=0), dict(h=-3), dict(w=8.0), dict(h=True), dict(frames=0), dict(frames=4097), dict(frames=2.0), dict(albedo=0), dict(albedo=None),
    dict(nd=None), dict(nd="x"), dict(out=None), dict(out=1.5), dict(cameras=None), dict(cameras=2), dict(cameras="x"),
    dict(cameras=np.zeros((3, 22), np.float32)), dict(objects=-4), dict(motion=4096), dict(n_objects=3),
    dict(objects=4096, motion=8192, n_objects=-1), dict(objects=4096, motion=8192, n_objects=65535),
    dict(objects=4096, motion=8192, n_objects=2.0), dict(motion=8192, n_objects=2), dict(prev=()), dict(prev="camera"),
    dict(prev=(1, 4096)), dict(prev=(1, 0, 4096)), dict(prev=(1, 4096, 8192, 12288)), dict(objects=4096, prev=(1, 4096, 8192)),
    dict(objects=4096, prev=(1, 4096, 8192, None)), dict(prev=(None, 4096, 8192)),
    dict(depth_tolerance=-0.1), dict(normal_tolerance=float("inf")), dict(coverage_tolerance=float("nan")), dict(depth_tolerance="1"),
], ids=lambda a: ",".join("%s=%.20r" % kv for kv in a.items()))
def test_binding_checks_arguments_before_the_library(monkeypatch, args):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(w=16, h=8, frames=3, albedo=1 << 20, nd=2 << 20, out=3 << 20, cameras=3, objects=None, motion=None, n_objects=0, prev=None)
    a.update(args)
    if isinstance(a["cameras"], int):
        a["cameras"] = cameras(a["cameras"])
    if isinstance(a["prev"], tuple) and a["prev"] and a["prev"][0] == 1:
        a["prev"] = (cameras(1)[0],) + a["prev"][1:]
    kw = {k: a.pop(k) for k in list(a) if k in api.TEMPORAL_DEFAULTS}
    with pytest.raises(ValueError):
        api.motion_vectors_device(a["w"], a["h"], a["frames"], a["albedo"], a["nd"], a["out"], a["cameras"], objects_ptr=a["objects"],
                                  motion_ptr=a["motion"], n_objects=a["n_objects"], prev=a["prev"], **kw)


@pytest.mark.parametrize("objects", [0, 1])
def test_flow_kernels_in_the_code_object(code_object, objects):  # noqa: F811
    bodies, meta = code_object
    name = FLOW % objects
    assert name in meta and name in bodies, "the motion-vector kernel is missing from the shipped code object"
    body, m = bodies[name], meta[name]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert count(body, r"scratch_") == 0
    assert count(body, r"flat_") == 0, "a FLAT instruction: a global pointer lost its address space"
    assert m["group_segment_fixed_size"] == 0 and m["agpr_count"] == 0 and count(body, r"ds_") == 0
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64
    assert m["vgpr_count"] <= 64, "more vector registers than eight waves per SIMD leave"
    # the frame's constants are scalar loads beside those of the kernel's arguments: the table's 33 words come in wide loads
    assert count(body, r"s_load_dwordx(4|8|16)") >= 3
    assert count(body, r"buffer_|global_atomic") == 0
    # one 16-byte store per pixel; this pixel's planes and at most two loads per tap and plane, the 4-byte ids beside them
    assert count(body, r"global_store_dwordx4") == 1 and count(body, r"global_store") == 1
    loads = count(body, r"global_load")
    assert 2 + 4 * 2 <= loads <= 2 + 4 * 3 + objects * (1 + 4 + 1), loads


def test_exactly_the_new_kernels_and_every_count_unchanged(code_object):  # noqa: F811
    """(every other family: tests/test_isa_contract.py holds the library to exactly tests/kernel_manifest.py)"""
    _, meta = code_object
    assert sorted(n for n in meta if "Flow" in n) == sorted(family(FLOW))


REFUSALS = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from toypathtracer_amd import api as tpt
from temporal_lib import look_at_camera
lib = tpt.load_library()
F = "tptMotionVectorsDevice"
w, h, N = 16, 8, 33
plane_b = w * h * 16
def msg(): return lib.tptGetLastError().decode()
def ptr(x): return None if x is None else (x if isinstance(x, int) else x.ctypes.data)
cams = np.stack([look_at_camera([0.02 * j, 2.0, 3.0], [0.0, 0.0, 0.0], w, h) for j in range(N)])
pcam = look_at_camera([-0.02, 2.0, 3.0], [0.0, 0.0, 0.0], w, h)
ins = dict(albedo=np.full((N, h, w, 4), 2.25, np.float32), nd=np.full((N, h, w, 4), 3.25, np.float32),
           objects=np.full((N, h, w), 3, np.int32), motion=np.full((N, 5, 4), 0.5, np.float32),
           prev_albedo=np.full((h, w, 4), 5.25, np.float32), prev_nd=np.full((h, w, 4), 4.25, np.float32),
           prev_object=np.full((h, w), 4, np.int32))
before = {k: v.copy() for k, v in ins.items()}
out = np.full((N + 1, h, w, 4), np.nan, np.float32)
big = np.full((2 * N + 3, h, w, 4), np.nan, np.float32)
FIELDS = dict(w="screenWidth", h="screenHeight", n="nFrames", fl="flags", cams="cameras", albedo="deviceFrameAlbedo",
              nd="deviceFrameNormalDepth", objects="deviceFrameObjects", motion="deviceFrameObjectMotion", out="deviceFrameMotion",
              pcam="prevCamera", prev_albedo="devicePrevAlbedo", prev_nd="devicePrevNormalDepth", prev_object="devicePrevObject",
              no="nObjects", dt="depthTolerance", nt="normalTolerance", ct="coverageTolerance")
BASE = dict(w=w, h=h, n=3, fl=0, cams=cams, albedo=ins["albedo"], nd=ins["nd"], objects=None, motion=None, out=out, pcam=None,
            prev_albedo=None, prev_nd=None, prev_object=None, no=0, dt=0.1, nt=0.25, ct=0.0)
OBJECTS = dict(objects=ins["objects"], motion=ins["motion"], no=5)
CONTINUED = dict(pcam=pcam, prev_albedo=ins["prev_albedo"], prev_nd=ins["prev_nd"])
def call(**kw):
    a = dict(BASE); a.update(kw)
    A = tpt.MotionVectorsArgs()
    for k, v in a.items():
        setattr(A, FIELDS[k], ptr(v) if FIELDS[k].startswith(("device", "cameras", "prevCamera")) else v)
    keep = list(a.values())
    return lib.tptMotionVectorsDevice(C.byref(A))
def refused(what, expect=F, **kw):
    rc = call(**kw)
    assert rc != 0 and expect in msg(), (what, rc, msg())
    print("refused:", what, "--", msg())
def changed(c, k, v):
    c = c.copy(); c.reshape(-1)[k] = v; return c
refused("no context", "not initialised")
tpt.InitializeTest()
so = C.CDLL(tpt.library_path())
class Launch(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("frames", "width", "height", "nObjects")] + [(n, C.c_void_p) for n in (
        "albedo", "nd", "object", "prev_albedo", "prev_nd", "prev_object", "motion", "out", "consts")] + [("ran", C.c_int)]
so.hostemuFlowLaunch.restype = C.POINTER(Launch)
so.hostemuFlowLaunch.argtypes = [C.c_int]
NF = so.hostemuFlowConstsFloats()
assert NF == 33
so.hostemuFlowConstsSeen.restype = C.POINTER(C.c_float * NF)
so.hostemuFlowConstsSeen.argtypes = [C.c_int, C.c_int]
so.hostemuTemporalConsts.restype = C.POINTER(C.c_float * 34)
def launches(): return so.hostemuFlowLaunches()
def launch(k): return so.hostemuFlowLaunch(k).contents
def seen(k, frame): return np.array(so.hostemuFlowConstsSeen(k, frame).contents, np.float32)
def ops():
    st = (C.c_longlong * 2)(); so.hostemu_stats(st); return st[0]
rc = lib.tptMotionVectorsDevice(None)
assert rc != 0 and F in msg(), msg()
print("refused: args NULL --", msg())
for n in (0, -1, 4097):
    refused("nFrames %d" % n, n=n)
for ww, hh in ((0, h), (w, 0), (8193, 1), (1, 8193), (-4, -4)):
    refused("size %dx%d" % (ww, hh), w=ww, h=hh)
for fl in (1, 2, 0x80000000):
    refused("flags %#x" % fl, fl=fl)
for k in ("cams", "albedo", "nd", "out"):
    refused("%s NULL" % k, **{k: None})
# the prev set: all given or all NULL, the object plane counting exactly when the clip has object planes
for k in ("prev_albedo", "prev_nd", "prev_object"):
    refused("%s without prevCamera" % k, **{k: ins[k]})
    refused("%s without prevCamera, object planes given" % k, **dict(OBJECTS, **{k: ins[k]}))
for k in ("prev_albedo", "prev_nd"):
    refused("prevCamera without %s" % k, **dict(CONTINUED, **{k: None}))
refused("prevCamera alone", pcam=pcam)
refused("prevCamera and object planes without the prev object plane", **dict(CONTINUED, **OBJECTS))
refused("prevCamera and a prev object plane without object planes", **dict(CONTINUED, prev_object=ins["prev_object"]))
refused("a table without object planes", motion=ins["motion"], no=5)
for no in (-1, 65535, 1 << 30):
    refused("nObjects %d" % no, **dict(OBJECTS, no=no))
refused("a table without a count", **dict(OBJECTS, no=0))
refused("a count without a table", **dict(OBJECTS, motion=None))
for name in ("dt", "nt", "ct"):
    for v in (-1e-6, float("nan"), float("inf")):
        refused("%s %r" % (name, v), **{name: v})
# every camera the temporal passes refuse, in every record and in prevCamera
for j in (0, 1, 2):
    refused("camera %d field 5 = inf" % j, cams=changed(cams[:3], 22 * j + 5, np.inf))
    flat = cams[:3].copy(); flat[j, 6:9] = 0
    refused("camera %d: dot(H, H) == 0" % j, cams=flat)
    back = cams[:3].copy(); back[j, 18:21] *= -1
    refused("camera %d: f <= 0" % j, cams=back)
refused("prevCamera field 3 = nan", **dict(CONTINUED, pcam=changed(pcam, 3, np.nan)))
flat = pcam.copy(); flat[9:12] = 0
refused("prevCamera: dot(V, V) == 0", **dict(CONTINUED, pcam=flat))
# overlaps, each buffer at its full extent
b = big.ctypes.data
for k in ("albedo", "nd"):
    refused("out is %s" % k, out=ins[k])
    refused("out's last plane holds the head of %s" % k, out=b, **{k: b + 3 * plane_b - 4})
    refused("the last plane of %s holds out's head" % k, out=b + 3 * plane_b - 16, **{k: b})
refused("out holds the third object plane", **dict(OBJECTS, out=b, objects=b + 2 * w * h * 4))
refused("the object planes' tail holds out's head", **dict(OBJECTS, objects=b, out=b + 3 * w * h * 4 - 4))
refused("out holds the third table's last entry", **dict(OBJECTS, out=b + 16, motion=b + 16 - 3 * 5 * 16 + 12))
refused("out holds the prev albedo plane", **dict(CONTINUED, out=b, prev_albedo=b + 3 * plane_b - 4))
refused("out holds the prev normal/depth plane", **dict(CONTINUED, out=b + plane_b - 4, prev_nd=b))
refused("out holds the prev object plane", **dict(CONTINUED, **dict(OBJECTS, out=b + w * h * 4 - 4, prev_object=b)))
# two rules broken at once: the one that is checked first is the one reported
def order(expect, **kw):
    rc = call(**kw)
    assert rc != 0 and msg() == F + ": " + expect, (expect, sorted(kw), rc, msg())
    print("order:", sorted(kw), "--", expect)
order("deviceFrameObjectMotion needs deviceFrameObjects", motion=ins["motion"], no=-1)
order("nObjects must lie in 0..65534", **dict(OBJECTS, no=65535, dt=-1.0))
order("deviceFrameObjectMotion and nObjects must be given together", **dict(OBJECTS, no=0, dt=-1.0))
order("every tolerance must be finite and at least 0", dt=-1.0, out=ins["albedo"])
assert launches() == 0 and so.hostemuTemporalLaunches() == 0, "a refused call reached a launcher"
o0 = ops()
tpt.synchronize()
assert ops() == o0, "a refused call enqueued something"
assert np.isnan(out).all() and np.isnan(big).all(), "a refused call wrote"

# ---------------------------------------------------------------- the launch plan of accepted calls
A_, ND_, OBJ_, MO_, OUT_ = [ins[k].ctypes.data for k in ("albedo", "nd", "objects", "motion")] + [out.ctypes.data]
ids_b = w * h * 4
for n in (1, 2, 33):
    for continued in (False, True):
        for objects in (False, True):
            out[:] = np.nan
            l0, o0 = launches(), ops()
            kw = dict(OBJECTS if objects else {}, **(dict(CONTINUED, prev_object=ins["prev_object"] if objects else None) if continued else {}))
            assert call(n=n, **kw) == 0, msg()
            got = [launch(k) for k in range(l0, launches())]
            # one launch for the frames whose predecessor lies in the stacks, one more for a frame 0 with a prev set
            assert len(got) == (1 if continued else 0) + (1 if n > 1 else 0), (n, continued, len(got))
            assert ops() == o0, "the lazy schedule ran something before anyone waited"
            tpt.synchronize()
            # what ran: the launches, a zero fill where frame 0 has no predecessor, and -- only if anything was launched -- ONE copy of
            # the table and the record of its event
            assert ops() - o0 == len(got) + (0 if continued else 1) + (2 if got else 0), (n, continued, ops() - o0)
            tables = {L.consts - 132 * (0 if (continued and i == 0) else (1 if continued else 0)) for i, L in enumerate(got)}
            assert len(tables) <= 1, "the launches of one call read more than one table"
            if continued:
                L = got[0]
                assert (L.frames, L.width, L.height) == (1, w, h)
                assert (L.albedo, L.nd, L.out) == (A_, ND_, OUT_)
                assert (L.prev_albedo, L.prev_nd) == (ins["prev_albedo"].ctypes.data, ins["prev_nd"].ctypes.data)
                assert (L.object, L.prev_object) == ((OBJ_, ins["prev_object"].ctypes.data) if objects else (None, None))
                assert (L.motion, L.nObjects) == ((MO_, 5) if objects else (None, 0))
            else:
                assert out[0].tobytes() == bytes(plane_b), "frame 0 without a predecessor is not zeroed"
            if n > 1:
                L = got[-1]
                assert (L.frames, L.width, L.height) == (n - 1, w, h)
                assert (L.albedo, L.nd, L.out) == (A_ + plane_b, ND_ + plane_b, OUT_ + plane_b)
                assert (L.prev_albedo, L.prev_nd) == (A_, ND_)
                assert (L.object, L.prev_object) == ((OBJ_ + ids_b, OBJ_) if objects else (None, None))
                assert (L.motion, L.nObjects) == ((MO_ + 5 * 16, 5) if objects else (None, 0))
            assert np.isnan(out[1:]).all(), "the stand-in launcher writes nothing, and nothing else may"
            assert all(L.ran for L in got)
            print("accepted: %d frames%s%s" % (n, ", continued" if continued else "", ", object planes" if objects else ""))
assert call(n=3, objects=ins["objects"]) == 0 and launch(launches() - 1).nObjects == 0 and launch(launches() - 1).object == OBJ_ + ids_b, msg()
print("accepted: object planes without a table")

# every frame's record is what temporalConsts gives the temporal pass for the same pair of cameras, bit for bit
tins = [np.full((h, w, 4), 0.5 + k, np.float32) for k in range(8)]
touts = [np.full((h, w, 4), np.nan, np.float32) for k in range(4)]
def per_frame(cam, prev, tol):
    pl = [ptr(p) for p in tins[:4]] + ([ptr(p) for p in tins[4:]] if prev is not None else [None] * 4) + [ptr(p) for p in touts]
    assert lib.tptTemporalAccumulateDevice(w, h, ptr(cam), ptr(prev), *pl, 2.0, *tol) == 0, msg()
    return np.array(so.hostemuTemporalConsts().contents, np.float32)
def same_record(got, want):
    """tptFlowConsts against tptTemporalConsts: the 30 camera words, then the three tolerances (the temporal record's word 30 is maxHistory)"""
    return got[:30].tobytes() == want[:30].tobytes() and got[30:33].tobytes() == want[31:34].tobytes()
tol = (0.2, 0.3, 0.4)
l0 = launches()
assert call(n=33, dt=tol[0], nt=tol[1], ct=tol[2], **CONTINUED) == 0, msg()
tpt.synchronize()
assert launches() == l0 + 2
assert same_record(seen(l0, 0), per_frame(cams[0], pcam, tol)), "frame 0's record"
for j in range(1, 33):
    assert same_record(seen(l0 + 1, j - 1), per_frame(cams[j], cams[j - 1], tol)), "frame %d's record" % j
want = per_frame(cams[0], pcam, tol)
assert want[12:15].tobytes() == pcam[0:3].tobytes() and want[0:3].tobytes() == cams[0, 0:3].tobytes()
print("accepted: the constants of every frame")

# two calls back to back, their cameras different, nothing waited for in between: each launch finds its own call's records, whenever
# its copy runs -- and so through a third and a fourth call, which take the first two's places
other = np.stack([look_at_camera([0.5 + 0.03 * j, 1.0, 4.0], [0.0, 0.5, 0.0], w, h) for j in range(N)])
third = np.stack([look_at_camera([-0.5 - 0.01 * j, 3.0, 2.0], [0.0, 0.0, 0.5], w, h) for j in range(N)])
far = np.stack([look_at_camera([0.0, 2.0 + 0.01 * j, 3.0], [0.0, 0.0, 0.0], w, h) for j in range(70)])
# (the fifth call grows the table: 70 frames, on stacks of its own of 70 planes)
long = dict(albedo=np.full((70, h, w, 4), 2.25, np.float32), nd=np.full((70, h, w, 4), 3.25, np.float32),
            out=np.full((70, h, w, 4), np.nan, np.float32))
plans = [(cams, 3, {}), (other, 3, {}), (third, 2, {}), (cams[5:], 9, {}), (far, 70, long), (third, 2, {})]
l0, o0 = launches(), ops()
for cs, n, kw in plans[:2]:
    assert call(n=n, cams=cs, **kw) == 0, msg()
assert ops() == o0, "the first call's copy ran before the second call was enqueued: the schedule shows nothing"
for cs, n, kw in plans[2:]:
    assert call(n=n, cams=cs, **kw) == 0, msg()
tpt.synchronize()
assert launches() == l0 + len(plans)
for k, (cs, n, _) in enumerate(plans):
    L = launch(l0 + k)
    assert L.frames == n - 1 and L.ran
    for j in range(1, min(n, 65)):
        assert same_record(seen(l0 + k, j - 1), per_frame(cs[j], cs[j - 1], (0.1, 0.25, 0.0))), ("call %d, frame %d reads another call's record" % (k, j))
print("accepted: calls back to back")
assert all((ins[k] == before[k]).all() for k in ins) and np.isnan(big).all(), "a call wrote an input"
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_and_the_launch_plan_through_the_host_runtime():
    out = run_refusals(REFUSALS, "libtpt_hostemu_flow.so", ["hostemu_flow.cpp", "hostemu_temporal.cpp"])
    head = 2 + 3 + 5 + 3 + 4
    prev_set = 6 + 2 + 1 + 2
    tables = 1 + 3 + 2
    scalars_and_cameras = 9 + 9 + 2
    overlaps = 6 + 3 + 3
    assert out.count("refused:") == head + prev_set + tables + scalars_and_cameras + overlaps, out
    assert out.count("accepted:") == 12 + 1 + 1 + 1, out
    assert out.count("order:") == 4, out
    F = "tptMotionVectorsDevice: "
    assert refusal_messages(out) == {
        "tpt: not initialised (call tptInitialize / InitializeTest first)": 1,
        F + "args is required": 1,
        F + "nFrames must lie in 1..4096": 3,
        F + "w and h must lie in 1..8192": 5,
        F + "flags must be 0": 3,
        F + "cameras, deviceFrameAlbedo, deviceFrameNormalDepth and deviceFrameMotion are required": 4,
        F + "devicePrevAlbedo, devicePrevNormalDepth and devicePrevObject need prevCamera": 6,
        F + "prevCamera needs devicePrevAlbedo and devicePrevNormalDepth": 3,
        F + "with prevCamera, devicePrevObject must be given exactly when deviceFrameObjects is": 2,
        F + "deviceFrameObjectMotion needs deviceFrameObjects": 1,
        F + "nObjects must lie in 0..65534": 3,
        F + "deviceFrameObjectMotion and nObjects must be given together": 2,
        F + "every tolerance must be finite and at least 0": 9,
        F + "camera has a non-finite field, a degenerate frame or its frame behind its origin": 9,
        F + "prevCamera has a non-finite field, a degenerate frame or its frame behind its origin": 2,
        F + "deviceFrameMotion overlaps an input": 12,
    }


def test_a_build_without_the_launcher_refuses():
    refused_without_its_launcher('''
sys.path.insert(0, sys.argv[1] + "/tests")
from temporal_lib import look_at_camera
planes = [np.full((2, 8, 16, 4), 0.25, np.float32) for _ in range(2)] + [np.full((2, 8, 16, 4), np.nan, np.float32)]
cams = np.stack([look_at_camera([0.02 * j, 2.0, 3.0], [0.0, 0.0, 0.0], 16, 8) for j in range(2)])
A = tpt.MotionVectorsArgs(screenWidth=16, screenHeight=8, nFrames=2, cameras=cams.ctypes.data, deviceFrameAlbedo=planes[0].ctypes.data,
                          deviceFrameNormalDepth=planes[1].ctypes.data, deviceFrameMotion=planes[2].ctypes.data, depthTolerance=0.1)
rc = lib.tptMotionVectorsDevice(C.byref(A))
tpt.synchronize()
assert np.isnan(planes[2]).all()
''', "tptMotionVectorsDevice: this build has no motion-vector kernel")
