"""tptRectifyHistoryDevice without a GPU: the declaration, binding and export; the binding's argument checks; the gfx950 code of the
three instantiations of the kernel in the shipped library; and the refusals, driven through the host runtime compiled against
tests/hostemu (a refused call returns before anything is enqueued; the launcher is tests/hostemu_rectify.cpp, which counts, runs
nothing, and shows what the host handed it)."""
import ctypes as C
import os
import re

import pytest

from isa_lib import code_object, count, exported_symbols, header_params, no_library, refusal_messages, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import RECTIFY, family
from oracle_lib import ROOT

# the kernel's LDS in 16-byte slots: (64 + 2R) x (4 + 2R) raw pixels and twice (4 + 2R) x 64 row sums (tptRectifyLayout)
LDS_BYTES = {r: 16 * ((64 + 2 * r) * (4 + 2 * r) + 2 * (4 + 2 * r) * 64) for r in (1, 2, 3)}
# DESIGN.md 3.16 records these from the code object's notes: radius -> (vgpr_count, sgpr_count)
REGISTERS = {1: (40, 34), 2: (56, 36), 3: (72, 34)}


def test_header_declares_the_entry_point():
    assert header_params("tptRectifyHistoryDevice") == [
        "int w", "int h", "const float* deviceColour", "const float* deviceMoments", "const float* deviceAccColour",
        "const float* deviceAccMoments", "float* deviceOutColour", "float* deviceOutMoments", "float* deviceOutVariance", "int radius",
        "float gamma"]
    text = open(os.path.join(ROOT, "include", "tpt_hip.h")).read()
    doc = text[text.index("HISTORY RECTIFICATION"):text.index("TPT_API int tptRectifyHistoryDevice")]
    for words in ("PASS-THROUGH", "left to right", "bottom to top", "no FMA", "sums from +0", "lerp = (N - 1) / N", "byte for byte",
                  "not finite", "in place", "Refused"):
        assert words in doc, words


def test_binding_and_export():
    from toypathtracer_amd import api
    name = "tptRectifyHistoryDevice"
    assert name in api.C_ABI_SYMBOLS and callable(api.rectify_history_device)
    assert api.RECTIFY_DEFAULTS.keys() == {"radius", "gamma"}
    assert 1 <= api.RECTIFY_DEFAULTS["radius"] <= api.RECTIFY_MAX_RADIUS == 3 and api.RECTIFY_DEFAULTS["gamma"] >= 0
    lib = api.load_library()
    assert hasattr(lib, name)
    assert lib.tptRectifyHistoryDevice.argtypes == [C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_float]
    assert re.search(r"\bT %s\b" % name, exported_symbols(api.library_path()))
    import inspect
    defaults = {k: v.default for k, v in inspect.signature(api.rectify_history_device).parameters.items()}
    assert {k: defaults[k] for k in api.RECTIFY_DEFAULTS} == api.RECTIFY_DEFAULTS


@pytest.mark.parametrize("args", [
    dict(w=0), dict(h=-3), dict(w=8.0), dict(h=True), dict(colour=0), dict(colour=None), dict(moments=1.5), dict(acc_colour=None),
    dict(acc_moments=-16), dict(out_colour=0), dict(out_moments="x"), dict(out_variance=None), dict(radius=0), dict(radius=4),
    dict(radius=2.0), dict(radius=True), dict(gamma=-0.1), dict(gamma=float("inf")), dict(gamma=float("nan")), dict(gamma="1"),
], ids=lambda a: ",".join("%s=%.20r" % kv for kv in a.items()))
def test_binding_checks_arguments_before_the_library(monkeypatch, args):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(w=16, h=8, colour=4096, moments=8192, acc_colour=12288, acc_moments=16384, out_colour=20480, out_moments=24576,
             out_variance=28672)
    a.update(args)
    kw = {k: a.pop(k) for k in list(a) if k in api.RECTIFY_DEFAULTS}
    with pytest.raises(ValueError):
        api.rectify_history_device(a["w"], a["h"], a["colour"], a["moments"], a["acc_colour"], a["acc_moments"], a["out_colour"],
                                   a["out_moments"], a["out_variance"], **kw)


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_rectify_kernels_in_the_code_object(code_object, radius):  # noqa: F811
    bodies, meta = code_object
    name = RECTIFY % radius
    assert name in meta and name in bodies, "the rectification kernel is missing from the shipped code object"
    body, m = bodies[name], meta[name]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert count(body, r"scratch_") == 0
    assert count(body, r"flat_") == 0, "a FLAT instruction: a global pointer lost its address space"
    assert m["group_segment_fixed_size"] == LDS_BYTES[radius] == {1: 18624, 2: 25088, 3: 31680}[radius], m
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64 and m["agpr_count"] == 0
    staged = -(-(64 + 2 * radius) * (4 + 2 * radius) // 256)  # loads of a lane for the tile and its halo
    assert (m["vgpr_count"], m["sgpr_count"]) == REGISTERS[radius], m  # (what DESIGN.md 3.16 records)
    # the LDS, not the registers, bounds the occupancy: floor(160 KiB / LDS) workgroups of four waves a CU, one wave of each per SIMD
    assert 512 // m["vgpr_count"] >= (160 * 1024) // LDS_BYTES[radius] == {1: 8, 2: 6, 3: 5}[radius]
    # the LDS is read and written in 16-byte slots only; two barriers, and nothing leaves before the second
    # (a slot whose fourth component nobody reads -- the sums of squares -- is read as 12 bytes)
    assert count(body, r"ds_") == count(body, r"ds_write_b128|ds_read_b(128|96)") > 0
    assert count(body, r"ds_write_b128") == staged + 2 * -(-(4 + 2 * radius) * 64 // 256)
    assert count(body, r"s_barrier") == 2
    # global traffic: the pixel's three planes and the tile with its halo, one load per 16-byte pixel (the compiler leaves out the
    # components nobody reads: the colours' alpha, the moments' .zw), three 16-byte stores
    assert count(body, r"global_load_dwordx[234]") == count(body, r"global_load") == 3 + staged
    assert count(body, r"global_store_dwordx4") == count(body, r"global_store") == 3
    assert count(body, r"buffer_|global_atomic") == 0


def test_exactly_the_new_kernels_and_every_count_unchanged(code_object):  # noqa: F811
    """(every other family: tests/test_isa_contract.py holds the library to exactly tests/kernel_manifest.py)"""
    _, meta = code_object
    assert sorted(n for n in meta if "Rectify" in n) == sorted(family(RECTIFY))


REFUSALS = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
F = "tptRectifyHistoryDevice"
w, h = 16, 8
ins = [np.full((h, w, 4), 0.25 + k, np.float32) for k in range(4)]   # colour, moments, accColour, accMoments
outs = [np.full((h, w, 4), np.nan, np.float32) for k in range(3)]    # outColour, outMoments, outVariance
big = np.full((2 * h, w, 4), np.nan, np.float32)
ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
def msg(): return lib.tptGetLastError().decode()
def call(ww=w, hh=h, i={}, o={}, radius=2, gamma=1.0):
    planes = list(ins) + list(outs)
    for k, v in i.items(): planes[k] = v
    for k, v in o.items(): planes[4 + k] = v
    return lib.tptRectifyHistoryDevice(ww, hh, *[ptr(p) for p in planes], radius, gamma), [ptr(p) for p in planes]
def refused(what, expect=F, **kw):
    rc, _ = call(**kw)
    assert rc != 0 and expect in msg(), (what, rc, msg())
    print("refused:", what, "--", msg())
refused("no context", "not initialised")
tpt.InitializeTest()
for ww, hh in ((0, h), (w, 0), (-1, h), (8193, 1), (1, 8193)):
    refused("size %dx%d" % (ww, hh), ww=ww, hh=hh)
for k in range(4):
    refused("input %d NULL" % k, i={k: None})
for k in range(3):
    refused("output %d NULL" % k, o={k: None})
for r in (0, -1, 4, 1 << 20):
    refused("radius %d" % r, radius=r)
for g in (-1e-6, -1.0, float("nan"), float("inf"), -float("inf")):
    refused("gamma %r" % g, gamma=g)
# overlaps: every output with every input, but for the two exact in-place equalities
for o in range(3):
    for i in range(4):
        if (o, i) not in ((0, 2), (1, 3)):
            refused("output %d is input %d" % (o, i), o={o: ins[i]})
refused("outColour starts inside accColour", i={2: big}, o={0: big.ctypes.data + 16})
refused("accColour starts inside outColour", i={2: big.ctypes.data + 16 * (w * h - 1)}, o={0: big})
refused("outMoments overlaps accMoments' tail", i={3: big}, o={1: big.ctypes.data + 16 * (w * h - 1)})
refused("outVariance overlaps this frame's colour", i={0: big.ctypes.data + 16 * 5}, o={2: big})
refused("two outputs are one", o={0: outs[1]})
refused("outVariance is outColour, in place", i={2: outs[0]}, o={2: outs[0]})
refused("two outputs overlap", o={1: big, 2: big.ctypes.data + 16 * 5})
refused("both outputs are accColour", i={2: outs[0]}, o={1: outs[0]})
so = C.CDLL(tpt.library_path())
class Launch(C.Structure):
    _fields_ = [("planes", C.c_void_p * 7), ("width", C.c_int), ("height", C.c_int), ("radius", C.c_int), ("gamma", C.c_float),
                ("stream", C.c_void_p)]
so.hostemuRectifyLast.restype = C.POINTER(Launch)
launches = so.hostemuRectifyLaunches
assert launches() == 0, "a refused call reached the launcher"
n = 0
for kw in (dict(), dict(radius=1, gamma=0.0), dict(radius=3, gamma=3e38), dict(i={2: outs[0]}), dict(i={3: outs[1]}),
           dict(i={2: outs[0], 3: outs[1]}, radius=1, gamma=0.5), dict(ww=8192, hh=1), dict(ww=1, hh=8192)):
    if kw.get("ww"):
        wide = [np.zeros((kw["hh"], kw["ww"], 4), np.float32) for _ in range(7)]
        kw = dict(kw, i=dict(enumerate(wide[:4])), o=dict(enumerate(wide[4:])))
    rc, ptrs = call(**kw)
    assert rc == 0, (kw, msg())
    n += 1
    assert launches() == n, "an accepted call reaches the launcher once"
    L = so.hostemuRectifyLast().contents
    assert [L.planes[k] for k in range(7)] == ptrs, "the pointers it was given"
    assert (L.width, L.height, L.radius) == (kw.get("ww", w), kw.get("hh", h), kw.get("radius", 2))
    assert L.gamma == np.float32(kw.get("gamma", 1.0))
    print("accepted:", sorted(k for k in kw if k not in "io"), sorted(kw.get("i", {})))
tpt.synchronize()
assert all(np.isnan(o).all() for o in outs) and np.isnan(big).all(), "a refused call wrote an output"
assert all((p == 0.25 + k).all() for k, p in enumerate(ins)), "a call wrote an input"
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_through_the_host_runtime():
    out = run_refusals(REFUSALS, "libtpt_hostemu_rectify.so", ["hostemu_rectify.cpp"])
    assert out.count("refused:") == 1 + 5 + 4 + 3 + 4 + 5 + 10 + 8, out
    assert out.count("accepted:") == 8, out
    F = "tptRectifyHistoryDevice: "
    assert refusal_messages(out) == {
        "tpt: not initialised (call tptInitialize / InitializeTest first)": 1,
        F + "w and h must lie in 1..8192": 5,
        F + "this frame's colour and moments planes and the accumulated ones are required": 4,
        F + "the three output planes are required": 3,
        F + "radius must lie in 1..3": 4,
        F + "gamma must be finite and at least 0": 5,
        F + "an output overlaps an input (other than in place)": 16,
        F + "two outputs overlap": 2,
    }


NO_KERNEL = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
tpt.InitializeTest()
planes = [np.full((4, 8, 4), np.nan, np.float32) for _ in range(7)]
rc = lib.tptRectifyHistoryDevice(8, 4, *[p.ctypes.data for p in planes], 2, 1.0)
msg = lib.tptGetLastError().decode()
assert rc != 0 and "tptRectifyHistoryDevice: this build has no" in msg and "kernel" in msg, (rc, msg)
assert msg == "tptRectifyHistoryDevice: this build has no history rectification kernel", msg
assert all(np.isnan(p).all() for p in planes)
tpt.ShutdownTest()
print("ok")
'''


def test_a_build_without_the_launcher_loads_and_refuses():
    """the launcher is a weak symbol: a host runtime linked without it loads, and the call fails by name"""
    run_refusals(NO_KERNEL, "libtpt_hostemu.so")
