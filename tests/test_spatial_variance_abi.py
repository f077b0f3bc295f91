"""tptSpatialVarianceDevice without a GPU: the declaration, binding and export; the binding's argument checks; the gfx950 code of the six
instantiations of the kernel in the shipped library; and the refusals, driven through the host runtime compiled against tests/hostemu (a
refused call returns before anything is enqueued; the launcher is tests/hostemu_spatial_variance.cpp, which counts, runs nothing, and
shows what the host handed it)."""
import ctypes as C
import inspect
import os
import re

import pytest

from isa_lib import code_object, count, exported_symbols, header_params, no_library, refusal_messages, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import SPREAD, family
from oracle_lib import ROOT

NAME = "tptSpatialVarianceDevice"
# the kernel's LDS in 16-byte slots: (64 + 2R) x (4 + 2R) moments pixels and, with the guide, as many normal / depth pixels
# (tptSpreadLayout)
LDS_BYTES = {(r, g): 16 * (64 + 2 * r) * (4 + 2 * r) * (1 + g) for r in (1, 2, 3) for g in (0, 1)}
# DESIGN.md 3.18 records these from the code object's notes: (radius, guide) -> (vgpr_count, sgpr_count)
REGISTERS = {(1, 0): (21, 30), (2, 0): (29, 30), (3, 0): (37, 30), (1, 1): (37, 36), (2, 1): (53, 46), (3, 1): (67, 58)}
VARIANTS = [(r, g) for r in (1, 2, 3) for g in (0, 1)]


def test_header_declares_the_entry_point():
    assert header_params(NAME) == [
        "int screenWidth", "int screenHeight", "int nFrames", "const float* deviceFrameMoments", "const float* deviceFrameNormalDepth",
        "float* deviceFrameOutVariance", "float samplesPerFrame", "float minSamples", "int radius", "float sigmaNormal", "float sigmaDepth"]
    text = open(os.path.join(ROOT, "include", "tpt_hip.h")).read()
    doc = text[text.index("SPATIAL VARIANCE ESTIMATE"):text.index("TPT_API int " + NAME)]
    for words in ("PASS-THROUGH", "left to right", "bottom to top", "no FMA", "sums from +0", "correctly rounded division", "byte for byte",
                  "samplesPerFrame * N < minSamples", "formed in binary32", "never leaves its own", "{0, v/N, 0, N}", "No tap counted",
                  "den = den * (1 + (dz*dz) * id)", "+infinity", "tptDenoiseClipDevice", "v_0", "variance bytes", "Asynchronous", "Refused",
                  "nFrames outside 1..4096", "full extent"):
        assert words in doc, words


def test_binding_and_export():
    from toypathtracer_amd import api
    assert NAME in api.C_ABI_SYMBOLS and callable(api.spatial_variance_device)
    assert api.SPATIAL_VARIANCE_DEFAULTS == dict(min_samples=2.0, radius=1, sigma_normal=0.03, sigma_depth=0.5)
    assert api.SPATIAL_VARIANCE_MAX_RADIUS == 3
    lib = api.load_library()
    assert hasattr(lib, NAME)
    assert lib.tptSpatialVarianceDevice.argtypes == [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_float, C.c_float, C.c_int, C.c_float, C.c_float]
    assert re.search(r"\bT %s\b" % NAME, exported_symbols(api.library_path()))
    sig = inspect.signature(api.spatial_variance_device)
    assert list(sig.parameters)[:7] == ["w", "h", "moments_ptr", "out_variance_ptr", "normal_depth_ptr", "frames", "samples_per_frame"]
    defaults = {k: v.default for k, v in sig.parameters.items()}
    assert {k: defaults[k] for k in api.SPATIAL_VARIANCE_DEFAULTS} == api.SPATIAL_VARIANCE_DEFAULTS
    assert (defaults["normal_depth_ptr"], defaults["frames"], defaults["samples_per_frame"]) == (None, 1, 1.0)


@pytest.mark.parametrize("args", [
    dict(w=0), dict(h=-3), dict(w=8.0), dict(h=True), dict(moments=0), dict(moments=None), dict(moments=1.5), dict(out=None), dict(out=0),
    dict(out="x"), dict(normal_depth=-16), dict(normal_depth=2.5), dict(frames=0), dict(frames=4097), dict(frames=2.0), dict(frames=True),
    dict(samples_per_frame=0.5), dict(samples_per_frame=float("inf")), dict(samples_per_frame=float("nan")), dict(samples_per_frame="1"),
    dict(min_samples=0.5), dict(min_samples=float("nan")), dict(min_samples="2"), dict(min_samples=True), dict(radius=0), dict(radius=4),
    dict(radius=2.0), dict(radius=True), dict(sigma_normal=-0.1), dict(sigma_depth=float("inf")), dict(sigma_normal=float("nan")),
    dict(sigma_depth="1"),
], ids=lambda a: ",".join("%s=%.20r" % kv for kv in a.items()))
def test_binding_checks_arguments_before_the_library(monkeypatch, args):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(w=16, h=8, moments=4096, out=8192, normal_depth=12288)
    a.update(args)
    kw = {k: a.pop(k) for k in list(a) if k in api.SPATIAL_VARIANCE_DEFAULTS or k in ("frames", "samples_per_frame")}
    with pytest.raises(ValueError):
        api.spatial_variance_device(a["w"], a["h"], a["moments"], a["out"], a["normal_depth"], **kw)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "r%d_guide%d" % v)
def test_spread_kernels_in_the_code_object(code_object, variant):  # noqa: F811
    bodies, meta = code_object
    radius, guide = variant
    name = SPREAD % variant
    assert name in meta and name in bodies, "the kernel is missing from the shipped code object"
    body, m = bodies[name], meta[name]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert count(body, r"scratch_") == 0
    assert count(body, r"flat_") == 0, "a FLAT instruction: a global pointer lost its address space"
    assert m["group_segment_fixed_size"] == LDS_BYTES[variant], m
    assert LDS_BYTES[(3, 1)] == 22400 and LDS_BYTES[(1, 0)] == 6336
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64 and m["agpr_count"] == 0
    assert (m["vgpr_count"], m["sgpr_count"]) == REGISTERS[variant], m  # (what DESIGN.md 3.18 records)
    # eight waves a SIMD for every variant but the guided radius 3 (seven); the LDS leaves room for at least seven workgroups a CU
    assert 512 // (-(-m["vgpr_count"] // 8) * 8) >= (7 if variant == (3, 1) else 8) and (160 * 1024) // LDS_BYTES[variant] >= 7
    # staging: one 16-byte LDS store per plane and item of a lane, plus the vote's; three barriers (the vote written, the vote read,
    # the tile staged), and the pass-through path leaves after the first
    staged = -(-(64 + 2 * radius) * (4 + 2 * radius) // 256)
    assert count(body, r"ds_write") == count(body, r"ds_write_b128") == 1 + staged * (1 + guide)
    assert count(body, r"s_barrier") == 3
    # global traffic: the pixel's own moments, the staged moments (.xy) and guide pixels, one 16-byte store
    assert count(body, r"global_load") == 2 + staged * (1 + guide)  # (the pixel's own .xy and .w are two loads)
    assert count(body, r"global_load_dwordx4") == staged * guide
    assert count(body, r"global_store_dwordx4") == count(body, r"global_store") == 1
    assert count(body, r"buffer_|global_atomic") == 0
    # IEEE divisions only (no bare reciprocal stands for a quotient): every v_rcp_f32 belongs to a v_div_fixup_f32
    assert count(body, r"v_rcp_f32") == count(body, r"v_div_fixup_f32") == count(body, r"v_div_fmas_f32") > 0
    assert count(body, r"v_rcp_iflag|v_rsq|v_sqrt") == 0


def test_exactly_the_new_kernels_and_every_count_unchanged(code_object):  # noqa: F811
    """(every other family, and how many kernels there are: tests/test_isa_contract.py holds the library to exactly
    tests/kernel_manifest.py)"""
    _, meta = code_object
    assert sorted(n for n in meta if "Spread" in n) == sorted(family(SPREAD)) == sorted(SPREAD % v for v in VARIANTS)


REFUSALS = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
F = "tptSpatialVarianceDevice"
w, h, n = 16, 8, 3
mo = np.full((n, h, w, 4), 0.25, np.float32)
nd = np.full((n, h, w, 4), 0.5, np.float32)
out = np.full((n, h, w, 4), np.nan, np.float32)
big = np.full((2 * n, h, w, 4), np.nan, np.float32)
plane = 16 * w * h
ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
def msg(): return lib.tptGetLastError().decode()
def call(ww=w, hh=h, frames=n, m=mo, g=nd, o=out, spp=1.0, ms=2.0, radius=2, sn=0.03, sd=0.5):
    return lib.tptSpatialVarianceDevice(ww, hh, frames, ptr(m), ptr(g), ptr(o), spp, ms, radius, sn, sd)
def refused(what, expect=F, **kw):
    rc = call(**kw)
    assert rc != 0 and expect in msg(), (what, rc, msg())
    print("refused:", what, "--", msg())
refused("no context", "not initialised")
tpt.InitializeTest()
for ww, hh in ((0, h), (w, 0), (-1, h), (8193, 1), (1, 8193)):
    refused("size %dx%d" % (ww, hh), ww=ww, hh=hh)
for f in (0, -1, 4097, 1 << 30):
    refused("nFrames %d" % f, frames=f)
refused("moments NULL", m=None)
refused("output NULL", o=None)
for r in (0, -1, 4, 1 << 20):
    refused("radius %d" % r, radius=r)
for s in (0.5, 0.0, -1.0, float("nan"), float("inf")):
    refused("samplesPerFrame %r" % s, spp=s)
for s in (0.5, 0.0, -float("inf"), float("nan")):
    refused("minSamples %r" % s, ms=s)
for kw in (dict(sn=-0.03), dict(sd=float("nan")), dict(sn=float("inf")), dict(sd=1e-7), dict(sn=1e7)):
    refused("sigma %r" % kw, **kw)
refused("sigmaNormal without the plane", g=None, sd=0.0)
refused("sigmaDepth without the plane", g=None, sn=0.0)
# overlaps, each plane taken at its full extent of nFrames planes
refused("output is the moments", o=mo)
refused("output is the guide", o=nd)
refused("output starts in the moments' last plane", m=big, o=big.ctypes.data + 3 * plane - 16)
refused("moments start in the output's last plane", m=big.ctypes.data + 3 * plane - 16, o=big)
refused("output's last pixel is the guide's first", g=big.ctypes.data + 3 * plane - 16, o=big)
refused("guide's last pixel is the output's first", g=big, o=big.ctypes.data + 3 * plane - 16)
so = C.CDLL(tpt.library_path())
class Launch(C.Structure):
    _fields_ = [("planes", C.c_void_p * 3), ("width", C.c_int), ("height", C.c_int), ("frames", C.c_int), ("radius", C.c_int),
                ("spp", C.c_float), ("ms", C.c_float), ("inn", C.c_float), ("idd", C.c_float), ("grid", C.c_uint * 3), ("stream", C.c_void_p)]
so.hostemuSpreadLast.restype = C.POINTER(Launch)
# two rules broken at once: the one that is checked first is the one reported
def order(expect, **kw):
    rc = call(**kw)
    assert rc != 0 and msg() == F + ": " + expect, (expect, kw, rc, msg())
    print("order:", sorted(kw), "--", expect)
order("radius must lie in 1..3", radius=0, spp=0.0)
order("samplesPerFrame must be finite and at least 1", spp=float("nan"), ms=0.0)
order("minSamples must be at least 1 (+infinity: every pixel is estimated)", ms=0.5, sn=float("nan"))
order("sigmaNormal and sigmaDepth must be 0 or lie in [1e-6, 1e6]", sd=2e6, g=None)
order("sigmaNormal and sigmaDepth need deviceFrameNormalDepth", g=None, o=mo)
launches = so.hostemuSpreadLaunches
assert launches() == 0, "a refused call reached the launcher"
f32 = np.float32
inv2 = lambda s: float(f32(1) / (f32(s) * f32(s))) if s > 0 else 0.0
count = 0
wide = np.zeros((1, 8192, 4), np.float32)
for kw in (dict(), dict(radius=1, frames=1), dict(radius=3, ms=float("inf")), dict(g=None, sn=0.0, sd=0.0), dict(sn=0.0, sd=0.0),
           dict(sn=1e-6, sd=1e6, spp=3e38, ms=1.0), dict(sn=0.0, sd=2.0, spp=4.0, ms=4.0),
           dict(m=big, o=big.ctypes.data + 3 * plane, g=None, sn=0.0, sd=0.0),
           dict(ww=8192, hh=1, frames=1, m=wide, g=None, o=wide.copy(), sn=0.0, sd=0.0),
           dict(ww=1, hh=8192, frames=1, m=wide, g=wide.copy(), o=wide.copy()), dict(ww=65, hh=5, frames=1), dict(ww=17, hh=5, frames=2)):
    k = dict(ww=w, hh=h, frames=n, m=mo, g=nd, o=out, spp=1.0, ms=2.0, radius=2, sn=0.03, sd=0.5)
    k.update(kw)
    rc = call(**k)
    assert rc == 0, (kw, msg())
    count += 1
    assert launches() == count, "an accepted call reaches the launcher once"
    L = so.hostemuSpreadLast().contents
    assert [L.planes[i] for i in range(3)] == [ptr(k["m"]), ptr(k["g"]), ptr(k["o"])], "the pointers it was given"
    assert (L.width, L.height, L.frames, L.radius) == (k["ww"], k["hh"], k["frames"], k["radius"])
    assert L.spp == f32(k["spp"]) and L.ms == f32(k["ms"])
    assert (L.inn, L.idd) == (inv2(k["sn"]), inv2(k["sd"])), "1 / sigma^2 in binary32, 0 for a sigma of 0"
    assert list(L.grid) == [(k["ww"] + 63) // 64, (k["hh"] + 3) // 4, k["frames"]], "64 x 4 pixels a workgroup, a frame per grid.z"
    print("accepted:", sorted(kw))
tpt.synchronize()
assert np.isnan(out).all() and np.isnan(big).all(), "a refused call wrote an output"
assert (mo == 0.25).all() and (nd == 0.5).all(), "a call wrote an input"
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_through_the_host_runtime():
    out = run_refusals(REFUSALS, "libtpt_hostemu_spatial_variance.so", ["hostemu_spatial_variance.cpp"])
    assert out.count("refused:") == 1 + 5 + 4 + 2 + 4 + 5 + 4 + 5 + 2 + 6, out
    assert out.count("accepted:") == 12, out
    assert out.count("order:") == 5, out
    F = "tptSpatialVarianceDevice: "
    assert refusal_messages(out) == {
        "tpt: not initialised (call tptInitialize / InitializeTest first)": 1,
        F + "screenWidth and screenHeight must lie in 1..8192": 5,
        F + "nFrames must lie in 1..4096": 4,
        F + "deviceFrameMoments and deviceFrameOutVariance are required": 2,
        F + "radius must lie in 1..3": 4,
        F + "samplesPerFrame must be finite and at least 1": 5,
        F + "minSamples must be at least 1 (+infinity: every pixel is estimated)": 4,
        F + "sigmaNormal and sigmaDepth must be 0 or lie in [1e-6, 1e6]": 5,
        F + "sigmaNormal and sigmaDepth need deviceFrameNormalDepth": 2,
        F + "deviceFrameOutVariance overlaps an input": 6,
    }


NO_KERNEL = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
tpt.InitializeTest()
planes = [np.full((4, 8, 4), np.nan, np.float32) for _ in range(3)]
rc = lib.tptSpatialVarianceDevice(8, 4, 1, *[p.ctypes.data for p in planes], 1.0, 2.0, 1, 0.03, 0.5)
msg = lib.tptGetLastError().decode()
assert rc != 0 and "tptSpatialVarianceDevice: this build has no" in msg and "kernel" in msg, (rc, msg)
assert msg == "tptSpatialVarianceDevice: this build has no spatial variance kernel", msg
assert all(np.isnan(p).all() for p in planes)
tpt.ShutdownTest()
print("ok")
'''


def test_a_build_without_the_launcher_loads_and_refuses():
    """the launcher is a weak symbol: a host runtime linked without it loads, and the call fails by name"""
    run_refusals(NO_KERNEL, "libtpt_hostemu.so")
