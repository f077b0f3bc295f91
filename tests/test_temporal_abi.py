"""tptTemporalAccumulateDevice without a GPU: the declaration, binding and export; the binding's argument checks; the gfx950 code of
the two instantiations of the kernel in the shipped library; and the refusals, driven through the host runtime compiled against
tests/hostemu (a refused call returns before anything is enqueued; the launcher is tests/hostemu_temporal.cpp, which counts and runs
nothing, and shows what the host made of the cameras)."""
import re

import numpy as np
import pytest

from isa_lib import code_object, count, exported_symbols, header, header_params, no_library, refusal_messages, refused_without_its_launcher, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import TEMPORAL


def test_header_declares_the_entry_point():
    assert header_params("tptTemporalAccumulateDevice") == [
        "int screenWidth", "int screenHeight", "const void* camera", "const void* prevCamera", "const float* deviceColour",
        "const float* deviceAlbedo", "const float* deviceNormalDepth", "const float* deviceMoments", "const float* devicePrevColour",
        "const float* devicePrevAlbedo", "const float* devicePrevNormalDepth", "const float* devicePrevMoments", "float* deviceOutColour",
        "float* deviceOutAlbedo", "float* deviceOutMoments", "float* deviceOutVariance", "float maxHistory", "float depthTolerance",
        "float normalTolerance", "float coverageTolerance"]
    m = re.search(r"#define\s+TPT_TEMPORAL_SNAP\s+\(1\.0f\s*/\s*(\d+)\)", header())
    from temporal_lib import SNAP
    assert m and np.float32(1.0) / np.float32(m.group(1)) == SNAP


def test_binding_and_export():
    from toypathtracer_amd import api
    assert "tptTemporalAccumulateDevice" in api.C_ABI_SYMBOLS
    assert callable(api.temporal_accumulate_device)
    assert api.TEMPORAL_DEFAULTS.keys() == {"max_history", "depth_tolerance", "normal_tolerance", "coverage_tolerance"}
    lib = api.load_library()
    assert hasattr(lib, "tptTemporalAccumulateDevice")
    assert re.search(r"\bT tptTemporalAccumulateDevice\b", exported_symbols(api.library_path()))


def camera():
    from toypathtracer_amd import api
    return np.zeros(1, api.CAMERA_DT)


@pytest.mark.parametrize("args", [
    dict(w=0), dict(h=-3), dict(w=8.0), dict(h=True), dict(camera=None), dict(camera=np.zeros(22, np.float32)), dict(camera=b"x" * 88),
    dict(colour=0), dict(albedo=None), dict(nd=1.5), dict(mo=-16), dict(out_colour=0), dict(out_albedo=None), dict(out_moments="x"),
    dict(out_variance=0), dict(prev=()), dict(prev=(None, 1, 2, 3, 4)), dict(prev="camera"), dict(prev_ptr=0), dict(prev_ptr=None),
    dict(prev_ptr=2.0), dict(max_history=0.5), dict(max_history=65537), dict(max_history=float("nan")), dict(max_history=True),
    dict(max_history="4"), dict(depth_tolerance=-0.1), dict(normal_tolerance=float("inf")), dict(coverage_tolerance=float("nan")),
], ids=lambda a: ",".join("%s=%.20r" % kv for kv in a.items()))
def test_binding_checks_arguments_before_the_library(monkeypatch, args):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(w=16, h=8, camera=camera(), colour=4096, albedo=8192, nd=12288, mo=16384, out_colour=20480, out_albedo=24576,
             out_moments=28672, out_variance=32768, prev=(camera(), 36864, 40960, 45056, 49152))
    if "prev_ptr" in args:
        a["prev"] = (camera(), 36864, args.pop("prev_ptr"), 45056, 49152)
    a.update(args)
    kw = {k: a.pop(k) for k in list(a) if k in api.TEMPORAL_DEFAULTS}
    with pytest.raises(ValueError):
        api.temporal_accumulate_device(a["w"], a["h"], a["camera"], a["colour"], a["albedo"], a["nd"], a["mo"], a["out_colour"],
                                       a["out_albedo"], a["out_moments"], a["out_variance"], prev=a["prev"], **kw)


@pytest.mark.parametrize("history", [1, 0], ids=["history", "first-frame"])
def test_temporal_kernels_in_the_code_object(code_object, history):
    bodies, meta = code_object
    name = TEMPORAL % history
    assert name in meta and name in bodies, "the temporal kernel is missing from the shipped code object"
    body, m = bodies[name], meta[name]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert count(body, r"scratch_") == 0
    assert count(body, r"flat_") == 0, "a FLAT instruction: a global pointer lost its address space"
    assert count(body, r"ds_") == 0 and m["group_segment_fixed_size"] == 0 and m["agpr_count"] == 0
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64
    assert m["vgpr_count"] <= 64, m  # (eight waves per SIMD)
    assert count(body, r"global_store_dwordx4") == 4 and count(body, r"global_store") == 4
    assert count(body, r"global_atomic|buffer_") == 0
    loads = count(body, r"global_load")
    if history:
        assert loads > 4  # this frame's four planes, and per tap the four of the history
    else:
        assert loads <= 4, "the first-frame form reads more than this frame's planes"
        assert count(body, r"v_sqrt|v_rsq") == 0  # (and projects nothing)


REFUSALS = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from toypathtracer_amd import api as tpt
from temporal_lib import look_at_camera
lib = tpt.load_library()
w, h = 16, 8
cam = look_at_camera([0.0, 2.0, 3.0], [0.0, 0.0, 0.0], w, h)
pcam = look_at_camera([0.1, 2.0, 3.0], [0.0, 0.0, 0.0], w, h)
ins = [np.full((h, w, 4), 0.25 + k, np.float32) for k in range(8)]
outs = [np.full((h, w, 4), np.nan, np.float32) for k in range(4)]
big = np.full((2 * h, w, 4), np.nan, np.float32)
ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
def call(ww=w, hh=h, c=cam, pc=pcam, i={}, o={}, mh=4.0, dt=0.1, nt=0.25, ct=0.0):
    planes = list(ins) + list(outs)
    for k, v in i.items(): planes[k] = v
    for k, v in o.items(): planes[8 + k] = v
    return lib.tptTemporalAccumulateDevice(ww, hh, ptr(c), ptr(pc), *[ptr(p) for p in planes], mh, dt, nt, ct)
def refused(what, expect="tptTemporalAccumulateDevice", **kw):
    rc = call(**kw)
    msg = lib.tptGetLastError().decode()
    assert rc != 0 and expect in msg, (what, rc, msg)
    print("refused:", what, "--", msg)
def changed(c, k, v):
    c = c.copy(); c[k] = v; return c
refused("no context", "not initialised")
tpt.InitializeTest()
for ww, hh in ((0, h), (w, 0), (8193, 1), (1, 8193)):
    refused("size %dx%d" % (ww, hh), ww=ww, hh=hh)
refused("camera NULL", c=None)
for k in range(4):
    refused("current plane %d NULL" % k, i={k: None})
    refused("output %d NULL" % k, o={k: None})
refused("prevCamera alone NULL", pc=None)
for k in range(4, 8):
    refused("prev plane %d alone NULL" % k, i={k: None})
refused("prevCamera alone given", i={4: None, 5: None, 6: None, 7: None})
for k in range(8):
    refused("output %d is input %d" % (k % 4, k), o={k % 4: ins[k]})
refused("an output overlaps an input's tail", i={2: big}, o={1: big.ctypes.data + 16 * (w * h - 1)})
refused("an output overlaps a prev plane's head", i={5: big.ctypes.data + 16 * (w * h - 1)}, o={3: big})
refused("two outputs are one", o={0: outs[1]})
refused("two outputs overlap", o={2: big, 3: big.ctypes.data + 16 * 5})
for mh in (0.0, 0.999, -4.0, 65536.5, float("nan"), float("inf")):
    refused("maxHistory %r" % mh, mh=mh)
for name in ("dt", "nt", "ct"):
    for v in (-1e-6, float("nan"), float("inf"), -float("inf")):
        refused("%s %r" % (name, v), **{name: v})
for which in ("c", "pc"):
    base = cam if which == "c" else pcam
    for k, v in ((0, np.nan), (5, np.inf), (13, -np.inf), (21, np.nan)):
        refused("%s field %d = %r" % (which, k, v), **{which: changed(base, k, v)})
    flat, thin, behind = base.copy(), base.copy(), base.copy()
    flat[6:9] = 0; thin[9:12] = 0; behind[18:21] = -behind[18:21]
    refused(which + ": dot(H, H) == 0", **{which: flat})
    refused(which + ": dot(V, V) == 0", **{which: thin})
    refused(which + ": f <= 0", **{which: behind})
so = C.CDLL(tpt.library_path())
launches = so.hostemuTemporalLaunches
so.hostemuTemporalConsts.restype = C.POINTER(C.c_float * 34)
assert launches() == 0, "a refused call reached the launcher"
first = dict(pc=None, i={4: None, 5: None, 6: None, 7: None})
for kw in (dict(), first, dict(mh=1.0), dict(mh=65536.0), dict(dt=0.0, nt=0.0, ct=0.0), dict(dt=3e38, nt=3e38, ct=3e38),
           dict(ww=8192, hh=1), dict(pc=cam)):
    if kw.get("ww") == 8192:
        wide = [np.zeros((1, 8192, 4), np.float32) for _ in range(12)]
        kw = dict(kw, i=dict(enumerate(wide[:8])), o=dict(enumerate(wide[8:])))
    assert call(**kw) == 0, (kw, lib.tptGetLastError().decode())
    print("accepted:", sorted(kw))
assert launches() == 8
# what the host made of the cameras of the last call (pc = cam): this camera's fields, a = ll' - o', f = -dot(a, w'), dot(H', H'), dot(V', V')
k = np.array(so.hostemuTemporalConsts().contents, np.float32)
a = cam[3:6] - cam[0:3]
dot = lambda u, v: np.float32(np.float32(u[0] * v[0] + u[1] * v[1]) + u[2] * v[2])
want = np.concatenate([cam[0:12], cam[0:3], a, cam[18:21], cam[6:12], [-dot(a, cam[18:21]), dot(cam[6:9], cam[6:9]), dot(cam[9:12], cam[9:12])],
                       [4.0, 0.1, 0.25, 0.0]]).astype(np.float32)
assert k.tobytes() == want.tobytes(), (k, want)
tpt.synchronize()
assert all(np.isnan(o).all() for o in outs) and np.isnan(big).all(), "a refused call wrote an output"
assert all((p == 0.25 + n).all() for n, p in enumerate(ins)), "a call wrote an input"
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_through_the_host_runtime(tmp_path):
    out = run_refusals(REFUSALS, "libtpt_hostemu_temporal.so", ["hostemu_temporal.cpp"])
    assert out.count("refused:") == 1 + 4 + 1 + 8 + 1 + 4 + 1 + 8 + 4 + 6 + 12 + 2 * 7, out
    assert out.count("accepted:") == 8, out
    F = "tptTemporalAccumulateDevice: "
    assert refusal_messages(out) == {
        "tpt: not initialised (call tptInitialize / InitializeTest first)": 1,
        F + "w and h must lie in 1..8192": 4,
        F + "camera is required": 1,
        F + "the four planes of this frame are required": 4,
        F + "the four output planes are required": 4,
        F + "prevCamera and the four prev planes must be all NULL or all given": 6,
        F + "an output overlaps an input": 10,
        F + "two outputs overlap": 2,
        F + "maxHistory must lie in 1..65536": 6,
        F + "every tolerance must be finite and at least 0": 12,
        F + "camera has a non-finite field, a degenerate frame or its frame behind its origin": 7,
        F + "prevCamera has a non-finite field, a degenerate frame or its frame behind its origin": 7,
    }


def test_a_build_without_the_launcher_refuses():
    refused_without_its_launcher('''
sys.path.insert(0, sys.argv[1] + "/tests")
from temporal_lib import look_at_camera
cam = look_at_camera([0.0, 2.0, 3.0], [0.0, 0.0, 0.0], 16, 8)
ins, outs = [np.full((8, 16, 4), 0.25, np.float32) for _ in range(4)], [np.full((8, 16, 4), np.nan, np.float32) for _ in range(4)]
rc = lib.tptTemporalAccumulateDevice(16, 8, cam.ctypes.data, None, *[p.ctypes.data for p in ins], None, None, None, None,
                                     *[p.ctypes.data for p in outs], 4.0, 0.1, 0.25, 0.0)
tpt.synchronize()
assert all(np.isnan(p).all() for p in outs)
''', "tptTemporalAccumulateDevice: this build has no temporal accumulation kernel")
