"""tptDrawDeviceMoments and tptDenoiseDeviceVariance without a GPU: the declarations, bindings and exports; the bindings' argument
checks and moment_samples; the gfx950 code of the new kernels in the shipped library (tests/test_aov_abi.py's contract for the trace
kernel, tests/test_denoise_abi.py's for the filter); and the refusals, driven through the host runtime compiled against tests/hostemu
(a refused call returns before anything is enqueued; the filter's launcher is tests/hostemu_variance.cpp, which counts and runs
nothing)."""
import re

import pytest

from isa_lib import code_object, count, exported_symbols, header, header_params, no_library, refusal_messages, refused_without_its_launcher, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import AOV, MOMENTS, QUEUE, VARIANCE, family


def test_header_declares_the_entry_points():
    assert header_params("tptDrawDeviceMoments") == ["float time", "int frameCount", "int screenWidth", "int screenHeight", "float* deviceTile",
                                              "float* deviceAlbedo", "float* deviceNormalDepth", "float* deviceMoments",
                                              "unsigned testFlags"]
    assert header_params("tptDenoiseDeviceVariance") == ["int screenWidth", "int screenHeight", "const float* deviceColour",
                                                  "const float* deviceAlbedo", "const float* deviceNormalDepth",
                                                  "const float* deviceMoments", "float samples", "float* deviceOut", "int iterations",
                                                  "float sigmaLuminance", "float sigmaNormal", "float sigmaDepth", "unsigned denoiseFlags"]
    m = re.search(r"#define\s+TPT_DENOISE_VARIANCE_EPS\s+(\S+)", header())
    from moments_lib import EPS
    import numpy as np
    assert m and np.float32(m.group(1).rstrip("f")) == EPS


@pytest.mark.parametrize("name,fn", [("tptDrawDeviceMoments", "draw_device_moments"), ("tptDenoiseDeviceVariance", "denoise_device_variance")])
def test_binding_and_export(name, fn):
    from toypathtracer_amd import api
    assert name in api.C_ABI_SYMBOLS
    assert callable(getattr(api, fn))
    lib = api.load_library()
    assert hasattr(lib, name)
    assert re.search(r"\bT %s\b" % name, exported_symbols(api.library_path()))


@pytest.mark.parametrize("args", [
    dict(w=0), dict(h=-3), dict(w=8.0), dict(h=True), dict(tile=0), dict(tile=None), dict(tile=1.5),
    dict(mo=0), dict(mo=None), dict(mo="x"), dict(albedo="x"), dict(nd=-16), dict(nd=2.0),
], ids=lambda a: ",".join("%s=%r" % kv for kv in a.items()))
def test_draw_binding_checks_arguments_before_the_library(monkeypatch, args):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(w=16, h=8, tile=4096, mo=32768, albedo=8192, nd=16384)
    a.update(args)
    with pytest.raises(ValueError):
        api.draw_device_moments(0.0, 0, a["w"], a["h"], a["tile"], a["mo"], 2, albedo_ptr=a["albedo"], normal_depth_ptr=a["nd"])


@pytest.mark.parametrize("args", [
    dict(w=0), dict(iterations=0), dict(iterations=2.0), dict(colour=0), dict(out=None), dict(mo=None), dict(mo=0), dict(mo=-1),
    dict(samples=0.5), dict(samples=float("nan")), dict(samples=float("inf")), dict(samples=True), dict(samples="4"),
    dict(sigma_luminance=0.0), dict(sigma_luminance=-1.0), dict(sigma_luminance=2e6), dict(sigma_luminance=float("nan")),
    dict(sigma_normal=-1.0), dict(sigma_depth=float("inf")), dict(demodulate=True, albedo=None),
], ids=lambda a: ",".join("%s=%r" % kv for kv in a.items()))
def test_denoise_binding_checks_arguments_before_the_library(monkeypatch, args):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(w=16, h=8, colour=4096, mo=32768, samples=4.0, out=65536, albedo=8192, nd=16384)
    a.update(args)
    kw = {k: a.pop(k) for k in list(a) if k in ("iterations", "sigma_luminance", "sigma_normal", "sigma_depth", "demodulate")}
    with pytest.raises(ValueError):
        api.denoise_device_variance(a["w"], a["h"], a["colour"], a["mo"], a["samples"], a["out"], albedo_ptr=a["albedo"],
                                    normal_depth_ptr=a["nd"], **kw)


def test_moment_samples():
    from toypathtracer_amd import api
    assert api.moment_samples(4) == 4.0
    assert api.moment_samples(4, 0, api.kFlagProgressive) == 4.0
    assert api.moment_samples(4, 63, api.kFlagProgressive) == 256.0
    assert api.moment_samples(16, 9, 0) == 16.0  # (not progressive: each frame stands alone)
    with pytest.raises(ValueError):
        api.moment_samples(4, 5, api.kFlagProgressive | api.kFlagAnimate)  # (an animated caller passes its own count)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            api.moment_samples(bad)
    with pytest.raises(ValueError):
        api.moment_samples(4, -1, api.kFlagProgressive)
    assert api.DENOISE_VARIANCE_DEFAULTS.keys() == {"iterations", "sigma_luminance", "sigma_normal", "sigma_depth"}


@pytest.mark.parametrize("lds", [1, 0], ids=["lds-scene", "grouped"])
def test_moments_kernels_keep_the_queue_kernel_contract(code_object, lds):
    bodies, meta = code_object
    name, twin = MOMENTS % lds, QUEUE % (lds, 0)
    assert name in meta and name in bodies, "the moments kernel is missing from the shipped code object"
    body, m, t = bodies[name], meta[name], meta[twin]
    assert count(body, r"flat_") == 0, "a FLAT instruction: an LDS pointer lost its address space"
    assert m["agpr_count"] == 0
    assert m["max_flat_workgroup_size"] == 512 and m["wavefront_size"] == 64
    assert m["group_segment_fixed_size"] == t["group_segment_fixed_size"]  # (the sums live in global memory)
    assert m["vgpr_count"] <= (120 if lds else 128), m
    assert m["vgpr_spill_count"] <= 6 and m["private_segment_fixed_size"] <= 28, m
    assert count(body, r"scratch_store") == count(body, r"scratch_load") <= 3
    # the moment sums and the frame's moments: global stores beyond the AOV kernel's
    assert count(body, r"global_store_dwordx4") > count(bodies[AOV % lds], r"global_store_dwordx4")
    assert count(body, r"v_mfma") == count(bodies[twin], r"v_mfma")


@pytest.mark.parametrize("first,last,guide", [(f, l, g) for f in (1, 0) for l in (1, 0) for g in (1, 0)], ids=lambda v: str(v))
def test_variance_kernels_in_the_code_object(code_object, first, last, guide):
    bodies, meta = code_object
    name = VARIANCE % (first, last, guide)
    assert name in meta and name in bodies, "the variance a-trous kernel is missing from the shipped code object"
    body, m = bodies[name], meta[name]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    assert count(body, r"scratch_") == 0
    assert count(body, r"flat_") == 0, "a FLAT instruction: a global pointer lost its address space"
    assert m["group_segment_fixed_size"] == 0 and m["agpr_count"] == 0
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64
    # 25 taps, each a coalesced load of 16 B (+ the guide's 16 B), and the 8 neighbours of the variance blur (their .w alone, or the
    # moments and albedo they are made from)
    assert count(body, r"global_load_dwordx[34]") >= 25 * (1 + guide)
    assert count(body, r"global_load_dword") >= 25 * (1 + guide) + 8
    assert count(body, r"global_store_dwordx4") == 1
    assert count(body, r"v_rcp_f32") >= 25


def test_no_new_kernel_name_contains_test(code_object):
    """(that no kernel of the library is a unit-test kernel: tests/test_isa_contract.py)"""
    _, meta = code_object
    assert sorted(n for n in meta if "TraceMoments" in n or "VarianceAtrous" in n) == sorted(family(MOMENTS) + family(VARIANCE))


REFUSALS = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
lib.tptDrawDeviceMoments.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
lib.tptDenoiseDeviceVariance.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int,
                                         C.c_float, C.c_float, C.c_float, C.c_uint]
w, h = 16, 8
tile = np.full((h, w, 4), 7.25, np.float32)
alb = np.full((h, w, 4), 0.25, np.float32)
nd = np.full((h, w, 4), 3.0, np.float32)
mo = np.full((h, w, 4), 0.5, np.float32)
out = np.full((h, w, 4), np.nan, np.float32)
big = np.zeros((2 * h, w, 4), np.float32)
ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
def draw(ww=w, hh=h, t=tile, a=alb, n=nd, m=mo):
    return lib.tptDrawDeviceMoments(0.0, 0, ww, hh, ptr(t), ptr(a), ptr(n), ptr(m), 2)
def den(ww=w, hh=h, c=tile, a=alb, n=nd, m=mo, s=4.0, o=out, it=3, sl=4.0, sn=0.2, sd=0.5, fl=1):
    return lib.tptDenoiseDeviceVariance(ww, hh, ptr(c), ptr(a), ptr(n), ptr(m), s, ptr(o), it, sl, sn, sd, fl)
def refused(what, fn, expect, **kw):
    rc = fn(**kw)
    msg = lib.tptGetLastError().decode()
    assert rc != 0 and expect in msg, (what, rc, msg)
    print("refused:", what, "--", msg)
def reset():
    tpt.set_seed_mode(1); tpt.set_fold_mode(0); tpt.set_kernel_variant(0, 3, -1); tpt.set_row_shard(0, 1, 0); tpt.set_samples_per_pixel(4)
D, V = "tptDrawDeviceMoments", "tptDenoiseDeviceVariance"
refused("draw: no context", draw, "not initialised")
refused("denoise: no context", den, "not initialised")
tpt.InitializeTest()
# ---- the draw
refused("before any tptUpdate", draw, D)
tpt.UpdateTest(0.0, 0, w, h, 2)
refused("moments NULL", draw, D, m=None)
refused("tile NULL", draw, D, t=None)
refused("moments is the tile", draw, D, m=tile)
refused("moments is the albedo", draw, D, m=alb)
refused("moments is the normal/depth plane", draw, D, m=nd)
refused("moments overlaps the tile's tail", draw, D, t=big, m=big.ctypes.data + 16 * (w * h - 1))
refused("no tptUpdate at this size", draw, D, hh=h + 1)
tpt.UpdateTest(0.0, 0, 8200, 8, 2)
refused("wider than 8192", draw, D, ww=8200, hh=8)
tpt.UpdateTest(0.0, 0, w, h, 2)
tpt.set_seed_mode(0); refused("row-serial seeds", draw, D); reset()
tpt.set_fold_mode(1); refused("forward fold", draw, D); reset()
for hs, persist in ((0, 1), (1, 3)):
    tpt.set_kernel_variant(hs, persist, -1); refused("variant %d/%d" % (hs, persist), draw, D)
reset()
tpt.set_samples_per_pixel(2048); refused("2048 spp", draw, D); reset()
tpt.set_row_shard(8, 2, 0); refused("row sharding", draw, D); reset()
tpt.comm_init_loopback(2, 8); refused("communicator", draw, D); tpt.comm_destroy(); reset()
mirror = np.zeros((h, w, 4), np.float32)
tpt.set_tile_mirror(mirror.ctypes.data); refused("tile mirror", draw, D); tpt.set_tile_mirror(None)
# ---- the filter
for ww, hh in ((0, h), (8193, 1)):
    refused("size %dx%d" % (ww, hh), den, V, ww=ww, hh=hh)
refused("colour NULL", den, V, c=None)
refused("out NULL", den, V, o=None)
refused("moments NULL", den, V, m=None)
refused("out is the moments", den, V, o=mo)
refused("out overlaps the moments' tail", den, V, m=big, o=big.ctypes.data + 16 * (w * h - 1))
refused("out is the colour", den, V, o=tile)
for it in (0, 9):
    refused("iterations %d" % it, den, V, it=it)
for s in (0.0, 0.999, -4.0, float("nan"), float("inf")):
    refused("samples %r" % s, den, V, s=s)
for sl in (0.0, -0.0, -1.0, 1.000001e6, float("nan"), float("inf")):
    refused("sigmaLuminance %r" % sl, den, V, sl=sl)
for v in (-1.0, 1e-7, float("nan"), 2e6):
    refused("sigmaNormal %r" % v, den, V, sn=v)
refused("sigmaDepth without the plane", den, V, n=None, sn=0.0)
refused("demodulate without albedo", den, V, a=None)
refused("unknown flag", den, V, fl=2)
# two rules broken at once: the one that is checked first is the one reported
def order(expect, **kw):
    rc = den(**kw)
    msg = lib.tptGetLastError().decode()
    assert rc != 0 and msg == V + ": " + expect, (expect, kw, rc, msg)
    print("order:", sorted(kw), "--", expect)
order("deviceColour and deviceOut are required", c=None, m=None)
order("deviceMoments is required", m=None, o=tile)
order("deviceOut overlaps an input", o=mo, it=0)
order("iterations must lie in 1..8", it=0, s=0.0)
order("samples must be finite and at least 1", s=float("nan"), sl=0.0)
order("sigmaLuminance must lie in (0, 1e6]", sl=0.0, sn=float("nan"))
order("sigmaNormal and sigmaDepth must be 0 or lie in [1e-6, 1e6]", sd=2e6, n=None)
order("sigmaNormal and sigmaDepth need deviceNormalDepth", n=None, fl=2)
order("unknown flag bits", fl=3, a=None)
launches = C.CDLL(tpt.library_path()).hostemuVarianceLaunches
assert launches() == 0, "a refused call reached the launcher"
for kw in (dict(it=1), dict(it=8), dict(s=1.0), dict(s=3e38), dict(sl=1e6), dict(sl=1e-30), dict(a=None, fl=0),
           dict(n=None, sn=0.0, sd=0.0), dict(a=None, n=None, sn=0.0, sd=0.0, fl=0)):
    assert den(**kw) == 0, (kw, lib.tptGetLastError().decode())
    print("accepted:", sorted(kw))
assert launches() == 9
tpt.synchronize()
assert np.isnan(out).all(), "a refused call wrote deviceOut"
assert (tile == 7.25).all() and (alb == 0.25).all() and (nd == 3.0).all() and (mo == 0.5).all(), "a refused call wrote"
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_through_the_host_runtime(tmp_path):
    out = run_refusals(REFUSALS, "libtpt_hostemu_variance.so", ["hostemu_variance.cpp"])
    assert out.count("refused:") == 2 + 9 + 8 + 2 + 6 + 2 + 5 + 6 + 4 + 3, out
    assert out.count("accepted:") == 9, out
    assert out.count("order:") == 9, out
    assert refusal_messages(out) == {
        "tpt: not initialised (call tptInitialize / InitializeTest first)": 2,
        "tptDrawDeviceMoments: call tptUpdate (UpdateTest) at this size first": 2,
        "tptDrawDeviceMoments: bad arguments (deviceTile, deviceMoments, size)": 2,
        "tptDrawDeviceMoments: deviceMoments overlaps the tile or a plane": 4,
        "tptDrawDeviceMoments: frames of at most 8192 x 8192": 1,
        "tptDrawDeviceMoments: needs per-pixel seeds (tptSetSeedMode(1)); row-serial moments are not supported": 1,
        "tptDrawDeviceMoments: needs the recursive fold (tptSetFoldMode(0))": 1,
        "tptDrawDeviceMoments: needs the path-queue kernel (tptSetKernelVariant(0, 3, ..))": 2,
        "tptDrawDeviceMoments: at most 2047 samples per pixel (the path-queue kernel)": 1,
        "tptDrawDeviceMoments: not with row sharding or a communicator (sharded moments are not supported)": 2,
        "tptDrawDeviceMoments: not with a tile mirror (tptSetTileMirror)": 1,
        "tptDenoiseDeviceVariance: w and h must lie in 1..8192": 2,
        "tptDenoiseDeviceVariance: deviceColour and deviceOut are required": 2,
        "tptDenoiseDeviceVariance: deviceMoments is required": 1,
        "tptDenoiseDeviceVariance: deviceOut overlaps an input": 3,
        "tptDenoiseDeviceVariance: iterations must lie in 1..8": 2,
        "tptDenoiseDeviceVariance: samples must be finite and at least 1": 5,
        "tptDenoiseDeviceVariance: sigmaLuminance must lie in (0, 1e6]": 6,
        "tptDenoiseDeviceVariance: sigmaNormal and sigmaDepth must be 0 or lie in [1e-6, 1e6]": 4,
        "tptDenoiseDeviceVariance: sigmaNormal and sigmaDepth need deviceNormalDepth": 1,
        "tptDenoiseDeviceVariance: TPT_DENOISE_DEMODULATE needs deviceAlbedo": 1,
        "tptDenoiseDeviceVariance: unknown flag bits": 1,
    }


def test_a_build_without_the_variance_launcher_refuses():
    refused_without_its_launcher('''
planes = [np.zeros((8, 16, 4), np.float32) for _ in range(2)] + [np.full((8, 16, 4), np.nan, np.float32)]
lib.tptDenoiseDeviceVariance.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int,
                                         C.c_float, C.c_float, C.c_float, C.c_uint]
rc = lib.tptDenoiseDeviceVariance(16, 8, planes[0].ctypes.data, None, None, planes[1].ctypes.data, 4.0, planes[2].ctypes.data, 3, 4.0, 0.0, 0.0, 0)
tpt.synchronize()
assert np.isnan(planes[2]).all()
''', "tptDenoiseDeviceVariance: this build has no variance-guided a-trous kernel")
