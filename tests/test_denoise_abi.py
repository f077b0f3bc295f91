"""tptDenoiseDevice without a GPU: the declaration, the binding and the export of the entry point; the binding's argument checks; the
gfx950 code of the a-trous kernels in the shipped library; and every refusal of the ABI, driven through the host runtime compiled
against tests/hostemu (a refused call returns before anything is enqueued, so no kernel is emulated), and the growth of the scratch
plane between the calls of one sequence, for which tests/hostemu_denoise.cpp runs the filter and tests/denoise_checker.c says the image."""
import re

import pytest

from isa_lib import code_object, count, exported_symbols, header, header_params, no_library, refusal_messages, refused_without_its_launcher, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import DENOISE, family


def test_header_declares_the_entry_point():
    params = header_params("tptDenoiseDevice")
    assert params == ["int screenWidth", "int screenHeight", "const float* deviceColour", "const float* deviceAlbedo",
                      "const float* deviceNormalDepth", "float* deviceOut", "int iterations", "float sigmaColour", "float sigmaNormal",
                      "float sigmaDepth", "unsigned denoiseFlags"], params
    assert re.search(r"enum\s*\{\s*TPT_DENOISE_DEMODULATE\s*=\s*1\s*<<\s*0\s*\}\s*;", header())


def test_binding_and_export():
    from toypathtracer_amd import api
    assert "tptDenoiseDevice" in api.C_ABI_SYMBOLS
    assert callable(api.denoise_device) and api.DENOISE_DEMODULATE == 1
    lib = api.load_library()
    assert hasattr(lib, "tptDenoiseDevice")
    assert re.search(r"\bT tptDenoiseDevice\b", exported_symbols(api.library_path()))


@pytest.mark.parametrize("args", [
    dict(w=0), dict(h=-3), dict(w=8.0), dict(h=True), dict(iterations=0), dict(iterations=2.0), dict(iterations=True),
    dict(colour=0), dict(colour=None), dict(colour=1.5), dict(out=None), dict(out=0), dict(out="x"),
    dict(albedo=-16), dict(albedo=2.0), dict(nd="x"), dict(nd=True),
    dict(sigma_colour=-1.0), dict(sigma_normal=float("nan")), dict(sigma_depth=float("inf")), dict(sigma_colour="1"),
    dict(albedo=None, demodulate=True),
], ids=lambda a: ",".join("%s=%r" % kv for kv in a.items()))
def test_binding_checks_arguments_before_the_library(monkeypatch, args):
    """every bad argument raises ValueError in Python: the library is never reached (load_library would fail the test)"""
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(w=16, h=8, colour=4096, out=8192, albedo=16384, nd=32768, iterations=5, sigma_colour=1.0, sigma_normal=0.2,
             sigma_depth=0.5, demodulate=None)
    a.update(args)
    with pytest.raises(ValueError):
        api.denoise_device(a["w"], a["h"], a["colour"], a["out"], albedo_ptr=a["albedo"], normal_depth_ptr=a["nd"],
                           iterations=a["iterations"], sigma_colour=a["sigma_colour"], sigma_normal=a["sigma_normal"],
                           sigma_depth=a["sigma_depth"], demodulate=a["demodulate"])


def test_binding_passes_what_it_means(monkeypatch):
    """demodulate=None follows the albedo plane; the sigmas of a guide that is not given go to the library as 0"""
    from toypathtracer_amd import api
    calls = []

    class Lib:
        def tptDenoiseDevice(self, *a):
            calls.append(a)
            return 0

    monkeypatch.setattr(api, "load_library", lambda: Lib())
    api.denoise_device(16, 8, 4096, 8192, albedo_ptr=16384, normal_depth_ptr=32768, iterations=3, sigma_colour=0.5)
    api.denoise_device(16, 8, 4096, 8192, iterations=1)
    api.denoise_device(16, 8, 4096, 8192, albedo_ptr=16384, demodulate=False)
    (a0, a1, a2) = calls
    assert a0[6] == 3 and a0[7] == 0.5 and a0[8] > 0 and a0[9] > 0 and a0[10] == 1
    assert a1[3] is None and a1[4] is None and a1[8] == 0.0 and a1[9] == 0.0 and a1[10] == 0
    assert a2[3] is not None and a2[10] == 0


@pytest.mark.parametrize("first,last,guide", [(f, l, g) for f in (1, 0) for l in (1, 0) for g in (1, 0)],
                         ids=lambda v: str(v))
def test_denoise_kernels_in_the_code_object(code_object, first, last, guide):
    bodies, meta = code_object
    name = DENOISE % (first, last, guide)
    assert name in meta and name in bodies, "the a-trous kernel is missing from the shipped code object"
    body, m = bodies[name], meta[name]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    assert count(body, r"scratch_") == 0
    assert count(body, r"flat_") == 0, "a FLAT instruction: a global pointer lost its address space"
    assert m["group_segment_fixed_size"] == 0 and m["agpr_count"] == 0
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64
    # 25 taps, each one coalesced load of the colour's rgb (+ the albedo when the first iteration demodulates, + the guide's 16 B)
    assert count(body, r"global_load_dwordx[34]") >= 25 * (1 + guide)
    assert count(body, r"global_store_dwordx4") == 1
    # the weights' division: the 6-instruction form (v_rcp_f32) on every tap, hipcc's expansion only behind its range check
    assert count(body, r"v_rcp_f32") >= 25


def test_no_kernel_name_contains_test(code_object):
    """(that no kernel of the library is a unit-test kernel: tests/test_isa_contract.py)"""
    _, meta = code_object
    assert sorted(n for n in meta if "Denoise" in n) == sorted(family(DENOISE))


REFUSALS = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
lib.tptDenoiseDevice.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                 C.c_float, C.c_uint]
w, h = 16, 8
col = np.full((h, w, 4), 0.5, np.float32)
alb = np.full((h, w, 4), 0.25, np.float32)
nd = np.full((h, w, 4), 3.0, np.float32)
out = np.full((h, w, 4), np.nan, np.float32)
big = np.zeros((2 * h, w, 4), np.float32)  # (room for an output that overlaps the tail of an input)
def call(ww=w, hh=h, c=col, a=alb, n=nd, o=out, it=3, sc=1.0, sn=0.2, sd=0.5, fl=1):
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
    return lib.tptDenoiseDevice(ww, hh, ptr(c), ptr(a), ptr(n), ptr(o), it, sc, sn, sd, fl)
def refused(what, expect="tptDenoiseDevice", **kw):
    rc = call(**kw)
    msg = lib.tptGetLastError().decode()
    assert rc != 0 and expect in msg, (what, rc, msg)
    print("refused:", what, "--", msg)
refused("no context", expect="not initialised")
tpt.InitializeTest()
for ww, hh in ((0, h), (w, 0), (-1, h), (8193, 1), (1, 8193)):
    refused("size %dx%d" % (ww, hh), ww=ww, hh=hh)
refused("colour NULL", c=None)
refused("out NULL", o=None)
refused("out is the colour", o=col)
refused("out is the albedo", o=alb)
refused("out is the normal/depth plane", o=nd)
refused("out overlaps the colour's tail", c=big, o=big.ctypes.data + 16 * (w * h - 1))
refused("colour overlaps out's tail", c=big.ctypes.data + 16 * (w * h - 1), o=big, a=None, n=None, sn=0.0, sd=0.0, fl=0)
for it in (0, -1, 9):
    refused("iterations %d" % it, it=it)
for name in ("sc", "sn", "sd"):
    for v in (-1.0, -1e-7, float("nan"), float("inf"), float("-inf"), 1e-7, 5e-7, 1.000001e6, 1e30):
        refused("%s = %r" % (name, v), **{name: v})
refused("sigmaNormal without the plane", n=None, sd=0.0)
refused("sigmaDepth without the plane", n=None, sn=0.0)
refused("demodulate without albedo", a=None)
for fl in (2, 4, 0x80000000, 3):
    refused("flags %#x" % fl, fl=fl)
launches = C.CDLL(tpt.library_path()).hostemuDenoiseLaunches
assert launches() == 0, "a refused call reached the launcher"
# accepted at the edges: each reaches the launcher (tests/hostemu_denoise.cpp counts them and runs nothing, so out stays NaN)
for kw in (dict(ww=8192, hh=1, c=np.zeros((1, 8192, 4), np.float32), o=np.zeros((1, 8192, 4), np.float32), a=None, n=None, sn=0.0, sd=0.0, fl=0),
           dict(it=1), dict(it=8), dict(sc=0.0, sn=0.0, sd=0.0), dict(sc=1e-6, sn=1e6, sd=1e-6), dict(a=None, fl=0), dict(n=None, sn=0.0, sd=0.0),
           dict(sc=-0.0)):
    assert call(**kw) == 0, (kw, lib.tptGetLastError().decode())
    print("accepted:", sorted(kw))
assert launches() == 8
tpt.synchronize()
assert np.isnan(out).all(), "a refused call wrote deviceOut"
assert (col == 0.5).all() and (alb == 0.25).all() and (nd == 3.0).all()
tpt.ShutdownTest()
# two rules broken at once: the one that is checked first is the one reported
tpt.InitializeTest()
def order(expect, **kw):
    rc = call(**kw)
    msg = lib.tptGetLastError().decode()
    assert rc != 0 and msg == "tptDenoiseDevice: " + expect, (expect, kw, rc, msg)
    print("order:", sorted(kw), "--", expect)
order("w and h must lie in 1..8192", ww=0, c=None)
order("deviceColour and deviceOut are required", o=None, a=out)
order("deviceOut overlaps an input", o=col, it=0)
order("iterations must lie in 1..8", it=9, sc=-1.0)
order("every sigma must be 0 or lie in [1e-6, 1e6]", sd=float("nan"), n=None)
order("sigmaNormal and sigmaDepth need deviceNormalDepth", n=None, fl=2)
order("unknown flag bits", fl=3, a=None)
assert launches() == 8
# the scratch plane the iterations ping-pong through (Context::dDenoise) grows between the calls of one sequence: 8 x 8, 24 x 16, 8 x 8
# again with no wait in between, the launcher now running the filter as stream work (tests/hostemu_denoise.cpp).  The growth itself
# drains the context stream (under the lazy schedule nothing else runs the first call before its plane goes), and every image is
# tests/denoise_checker.c's.  Four iterations: the scratch plane is written, read, written and read again.
import tempfile
sys.path.insert(0, sys.argv[1] + "/tests")
from denoise_lib import DenoiseChecker, random_planes
checker = DenoiseChecker(tempfile.mkdtemp(prefix="denoise_abi_"))
emu = C.CDLL(tpt.library_path())
emu.hostemuDenoiseRun(1)
def stats():
    st = (C.c_longlong * 2)(); emu.hostemu_stats(st); return st[0], st[1]
rng = np.random.default_rng(11)
planes = [random_planes(rng, hh, ww) for ww, hh in ((8, 8), (24, 16), (8, 8))]
outs = [np.full(p[0].shape, np.nan, np.float32) for p in planes]
def run(k):
    c, a, n = planes[k]
    assert call(ww=c.shape[1], hh=c.shape[0], c=c, a=a, n=n, o=outs[k], it=4) == 0, lib.tptGetLastError().decode()
run(0)
ran, frees = stats()
run(1)
assert stats()[1] == frees + 1, "the scratch plane did not grow"
assert stats()[0] > ran, "the growth did not drain the context stream"
run(2)
assert stats()[1] == frees + 1, "the scratch plane was replaced again"
tpt.synchronize()
for k, (c, a, n) in enumerate(planes):
    want = checker.run(c, a, n, iterations=4, sigma_colour=1.0, sigma_normal=0.2, sigma_depth=0.5, flags=1)
    assert outs[k].tobytes() == want.tobytes(), ("growth", k)
print("growth: the scratch plane grows between calls")
tpt.ShutdownTest()
print("ok")
'''


def test_a_build_without_the_launcher_refuses():
    refused_without_its_launcher('''
col, out = np.zeros((8, 16, 4), np.float32), np.full((8, 16, 4), np.nan, np.float32)
lib.tptDenoiseDevice.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_uint]
rc = lib.tptDenoiseDevice(16, 8, col.ctypes.data, None, None, out.ctypes.data, 3, 1.0, 0.0, 0.0, 0)
tpt.synchronize()
assert np.isnan(out).all()
''', "tptDenoiseDevice: this build has no a-trous kernel")


def test_refusals_through_the_host_runtime(tmp_path):
    # (the host runtime with the counting launcher of tests/hostemu_denoise.cpp beside the emulated kernels)
    out = run_refusals(REFUSALS, "libtpt_hostemu_denoise.so", ["hostemu_denoise.cpp"])
    assert out.count("refused:") == 1 + 5 + 2 + 3 + 2 + 3 + 27 + 3 + 4, out
    assert out.count("accepted:") == 8, out
    assert out.count("order:") == 7 and "growth: the scratch plane grows between calls" in out, out
    assert refusal_messages(out) == {
        "tpt: not initialised (call tptInitialize / InitializeTest first)": 1,
        "tptDenoiseDevice: w and h must lie in 1..8192": 5,
        "tptDenoiseDevice: deviceColour and deviceOut are required": 2,
        "tptDenoiseDevice: deviceOut overlaps an input": 5,
        "tptDenoiseDevice: iterations must lie in 1..8": 3,
        "tptDenoiseDevice: every sigma must be 0 or lie in [1e-6, 1e6]": 27,
        "tptDenoiseDevice: sigmaNormal and sigmaDepth need deviceNormalDepth": 2,
        "tptDenoiseDevice: TPT_DENOISE_DEMODULATE needs deviceAlbedo": 1,
        "tptDenoiseDevice: unknown flag bits": 4,
    }
