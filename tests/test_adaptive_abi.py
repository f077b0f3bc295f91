"""tptDrawDeviceAdaptive and tptAdaptiveSamplesDevice without a GPU: the declarations, bindings and exports; the bindings' argument
checks; the gfx950 code of the new kernels in the shipped library -- the adaptive trace kernels held to their moments twins' contract,
and the existing instantiations of the path-queue kernel held to the register, spill and LDS figures they had before this variant was
compiled beside them --; and the refusals, driven through the host runtime compiled against tests/hostemu (a refused call returns
before anything is enqueued; the new launchers are tests/hostemu_adaptive.cpp, which counts and runs nothing)."""
import re

import pytest

from isa_lib import code_object, count, exported_symbols, header, header_params, no_library, refusal_messages, refused_without_its_launcher, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import ADAPTIVE, ADAPTIVE_PLAN as PLAN, ADAPTIVE_RESOLVE as RESOLVE, MOMENTS, QUEUE, family

# The path-queue kernel's instantiations as the parent commit's build has them (the same compiler, the same flags):
# (vgpr_count, group_segment_fixed_size, vgpr_spill_count, sgpr_spill_count, private_segment_fixed_size).  The adaptive variant is one
# more instantiation of the same template: compiled beside them it must leave them what they were.
PARENT = {
    "_ZN3tpt17tptTraceAovKernelILb0EEEvNS_10KernelArgsE": (128, 0, 6, 115, 28),
    "_ZN3tpt17tptTraceAovKernelILb1EEEvNS_10KernelArgsE": (119, 0, 4, 46, 20),
    "_ZN3tpt18tptTraceClipKernelILb0EEEvNS_10KernelArgsE": (91, 0, 0, 31, 0),
    "_ZN3tpt18tptTraceClipKernelILb1EEEvNS_10KernelArgsE": (120, 0, 4, 88, 20),
    "_ZN3tpt19tptTraceQueueKernelILb0ELb0EEEvNS_10KernelArgsE": (128, 0, 4, 103, 20),
    "_ZN3tpt19tptTraceQueueKernelILb0ELb1EEEvNS_10KernelArgsE": (128, 0, 6, 124, 28),
    "_ZN3tpt19tptTraceQueueKernelILb1ELb0EEEvNS_10KernelArgsE": (120, 0, 2, 33, 12),
    "_ZN3tpt19tptTraceQueueKernelILb1ELb1EEEvNS_10KernelArgsE": (120, 0, 2, 56, 12),
    "_ZN3tpt19tptTraceViewsKernelILb0EEEvNS_10KernelArgsE": (128, 0, 6, 122, 28),
    "_ZN3tpt19tptTraceViewsKernelILb1EEEvNS_10KernelArgsE": (120, 0, 2, 58, 12),
    "_ZN3tpt21tptTraceMomentsKernelILb0EEEvNS_10KernelArgsE": (128, 0, 6, 117, 28),
    "_ZN3tpt21tptTraceMomentsKernelILb1EEEvNS_10KernelArgsE": (119, 0, 4, 55, 20),
    "_ZN3tpt23tptTraceAnimationKernelILb0EEEvNS_10KernelArgsE": (89, 0, 0, 25, 0),
    "_ZN3tpt23tptTraceAnimationKernelILb1EEEvNS_10KernelArgsE": (120, 0, 2, 58, 12),
}


def test_header_declares_the_entry_points():
    assert header_params("tptDrawDeviceAdaptive") == ["float time", "int frameCount", "int screenWidth", "int screenHeight",
                                                      "float* deviceTile", "float* deviceAlbedo", "float* deviceNormalDepth",
                                                      "float* deviceMoments", "const int32_t* deviceSampleCounts", "unsigned testFlags"]
    assert header_params("tptAdaptiveSamplesDevice") == ["int screenWidth", "int screenHeight", "const float* deviceMoments",
                                                         "float targetError", "int minSamples", "int maxSamples",
                                                         "int32_t* deviceSampleCounts", "float* deviceOutVariance",
                                                         "int64_t* deviceTotalSamples"]
    m = re.search(r"#define\s+TPT_ADAPTIVE_LUM_FLOOR\s+(\S+)", header())
    from adaptive_lib import LUM_FLOOR
    import numpy as np
    assert m and np.float32(m.group(1).rstrip("f")) == LUM_FLOOR


@pytest.mark.parametrize("name,fn", [("tptDrawDeviceAdaptive", "draw_device_adaptive"), ("tptAdaptiveSamplesDevice", "adaptive_samples_device")])
def test_binding_and_export(name, fn):
    from toypathtracer_amd import api
    assert name in api.C_ABI_SYMBOLS
    assert callable(getattr(api, fn))
    lib = api.load_library()
    assert hasattr(lib, name)
    assert re.search(r"\bT %s\b" % name, exported_symbols(api.library_path()))


@pytest.mark.parametrize("args", [
    dict(w=0), dict(h=-3), dict(w=8.0), dict(h=True), dict(tile=0), dict(tile=None), dict(tile=1.5), dict(mo=0), dict(mo=None),
    dict(mo="x"), dict(counts=None), dict(counts=0), dict(counts=2.5), dict(albedo="x"), dict(nd=-16), dict(nd=2.0),
], ids=lambda a: ",".join("%s=%r" % kv for kv in a.items()))
def test_draw_binding_checks_arguments_before_the_library(monkeypatch, args):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(w=16, h=8, tile=4096, mo=32768, counts=65536, albedo=8192, nd=16384)
    a.update(args)
    with pytest.raises(ValueError):
        api.draw_device_adaptive(0.0, 0, a["w"], a["h"], a["tile"], a["mo"], a["counts"], 2, albedo_ptr=a["albedo"], normal_depth_ptr=a["nd"])


@pytest.mark.parametrize("args", [
    dict(w=0), dict(h=2.0), dict(mo=None), dict(mo=0), dict(counts=None), dict(counts=-4), dict(var="x"), dict(total=1.5),
    dict(te=0.0), dict(te=-0.1), dict(te=2e6), dict(te=float("nan")), dict(te=float("inf")), dict(te=True), dict(te="0.1"),
    dict(lo=-1), dict(lo=1.0), dict(hi=2048), dict(hi=True), dict(lo=9, hi=8),
], ids=lambda a: ",".join("%s=%r" % kv for kv in a.items()))
def test_plan_binding_checks_arguments_before_the_library(monkeypatch, args):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(w=16, h=8, mo=4096, te=0.05, counts=32768, lo=0, hi=64, var=65536, total=131072)
    a.update(args)
    with pytest.raises(ValueError):
        api.adaptive_samples_device(a["w"], a["h"], a["mo"], a["te"], a["counts"], min_samples=a["lo"], max_samples=a["hi"],
                                    out_variance_ptr=a["var"], total_ptr=a["total"])


# ---------------------------------------------------------------- the shipped gfx950 code
@pytest.mark.parametrize("lds", [1, 0], ids=["lds-scene", "grouped"])
def test_adaptive_trace_kernels_keep_their_moments_twins_contract(code_object, lds):  # noqa: F811
    bodies, meta = code_object
    name, twin = ADAPTIVE % lds, MOMENTS % lds
    assert name in meta and name in bodies, "the adaptive trace kernel is missing from the shipped code object"
    body, m, t = bodies[name], meta[name], meta[twin]
    assert count(body, r"flat_") == 0, "a FLAT instruction: an LDS pointer lost its address space"
    assert count(body, r"buffer_(load|store|atomic)") == 0
    assert m["group_segment_fixed_size"] == t["group_segment_fixed_size"]  # (the count travels in the sums, in global memory)
    assert m["agpr_count"] == 0
    assert m["max_flat_workgroup_size"] == 512 and m["wavefront_size"] == 64
    assert m["vgpr_count"] <= t["vgpr_count"], (m, t)
    assert m["vgpr_spill_count"] <= t["vgpr_spill_count"] and m["private_segment_fixed_size"] <= t["private_segment_fixed_size"], (m, t)
    assert count(body, r"v_mfma") == count(bodies[twin], r"v_mfma") == count(bodies[QUEUE % (lds, 0)], r"v_mfma")
    # the pixel's reciprocal is made in the kernel: one v_rcp_f32 more than the twin at least; no scalar-memory store or atomic anywhere
    assert count(body, r"v_rcp_f32") > count(bodies[twin], r"v_rcp_f32")
    assert count(body, r"s_(buffer_|scratch_)?(store|atomic)") == 0


def test_helper_kernels_in_the_code_object(code_object):  # noqa: F811
    bodies, meta = code_object
    for name, loads, stores in ((RESOLVE, 5, 2), (PLAN, 9, 2)):
        assert name in meta and name in bodies, "%s is missing from the shipped code object" % name
        body, m = bodies[name], meta[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["group_segment_fixed_size"] == 0, m
        assert m["agpr_count"] == 0 and m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64
        assert count(body, r"flat_") == 0 and count(body, r"scratch_") == 0
        assert count(body, r"global_load_dword") >= loads and count(body, r"global_store_dword") == stores
        assert count(body, r"s_(buffer_|scratch_)?(store|atomic)") == 0
    # the total: summed within the wave, then one 64-bit vector atomic
    assert count(bodies[PLAN], r"global_atomic_add_x2") == 1 and count(bodies[PLAN], r"global_atomic") == 1
    assert count(bodies[RESOLVE], r"global_atomic") == 0


def test_new_kernel_names_hold_no_counted_word(code_object):  # noqa: F811
    """(no test counts kernels by the words in their names any more: tests/test_isa_contract.py holds the library to the manifest)"""
    _, meta = code_object
    assert sorted(n for n in meta if "Adaptive" in n) == sorted(family(ADAPTIVE) + [RESOLVE, PLAN])


def test_existing_instantiations_are_what_the_parent_built(code_object):  # noqa: F811
    _, meta = code_object
    for name, want in PARENT.items():
        m = meta[name]
        got = (m["vgpr_count"], m["group_segment_fixed_size"], m["vgpr_spill_count"], m["sgpr_spill_count"], m["private_segment_fixed_size"])
        assert got == want, (name, got, want)


# ---------------------------------------------------------------- refusals, through the host runtime
REFUSALS = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
lib.tptDrawDeviceAdaptive.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_uint]
lib.tptAdaptiveSamplesDevice.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
w, h = 16, 8
plane = w * h * 16
tile = np.full((h, w, 4), 7.25, np.float32)
alb = np.full((h, w, 4), 0.25, np.float32)
nd = np.full((h, w, 4), 3.0, np.float32)
mo = np.full((h, w, 4), 0.5, np.float32)
cnt = np.full((h, w), 4, np.int32)
var = np.full((h, w, 4), -2.0, np.float32)
tot = np.full(1, -9, np.int64)
big = np.zeros((2 * h, w, 4), np.float32)
ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
def draw(ww=w, hh=h, t=tile, a=alb, n=nd, m=mo, c=cnt):
    return lib.tptDrawDeviceAdaptive(0.0, 0, ww, hh, ptr(t), ptr(a), ptr(n), ptr(m), ptr(c), 2)
def plan(ww=w, hh=h, m=mo, te=0.05, lo=0, hi=64, c=cnt, v=var, t=tot):
    return lib.tptAdaptiveSamplesDevice(ww, hh, ptr(m), te, lo, hi, ptr(c), ptr(v), ptr(t))
def refused(what, fn, expect, **kw):
    rc = fn(**kw)
    msg = lib.tptGetLastError().decode()
    assert rc != 0 and expect in msg, (what, rc, msg)
    print("refused:", what, "--", msg)
def reset():
    tpt.set_seed_mode(1); tpt.set_fold_mode(0); tpt.set_kernel_variant(0, 3, -1); tpt.set_row_shard(0, 1, 0); tpt.set_samples_per_pixel(4)
D, P = "tptDrawDeviceAdaptive", "tptAdaptiveSamplesDevice"
refused("draw: no context", draw, "not initialised")
refused("plan: no context", plan, "not initialised")
tpt.InitializeTest()
emu = C.CDLL(tpt.library_path())
# ---- the draw: what tptDrawDeviceMoments refuses ...
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
tpt.set_row_shard(8, 2, 0); refused("row sharding", draw, D); reset()
tpt.comm_init_loopback(2, 8); refused("communicator", draw, D); tpt.comm_destroy(); reset()
mirror = np.zeros((h, w, 4), np.float32)
tpt.set_tile_mirror(mirror.ctypes.data); refused("tile mirror", draw, D); tpt.set_tile_mirror(None)
# ---- ... and its own
refused("counts NULL", draw, D, c=None)
refused("counts in the tile", draw, D, c=tile.ctypes.data + 64)
refused("counts in the moments' last pixel", draw, D, c=mo.ctypes.data + plane - 4)
refused("counts in the albedo", draw, D, c=alb.ctypes.data)
refused("the normal/depth plane starts in the counts' last word", draw, D, t=big, n=big.ctypes.data + plane, c=big.ctypes.data + plane - w * h * 4 + 4)
assert emu.hostemuAdaptiveResolves() == 0, "a refused draw reached the launcher"
tpt.synchronize()
assert (tile == 7.25).all() and (alb == 0.25).all() and (nd == 3.0).all() and (mo == 0.5).all() and (cnt == 4).all(), "a refused call wrote"
assert (big == 0.0).all(), "a refused call wrote"
# ---- accepted: a context spp over 2047 plays no part; optional planes NULL; counts right behind a plane
tpt.set_samples_per_pixel(4096)
assert draw(a=None, n=None) == 0, lib.tptGetLastError().decode()
print("accepted: 4096 context spp, no planes")
assert emu.hostemuAdaptiveResolves() == 1
reset()
assert draw(t=big, c=big.ctypes.data + plane) == 0, lib.tptGetLastError().decode()
print("accepted: counts adjacent to the tile")
assert emu.hostemuAdaptiveResolves() == 2
tpt.synchronize()
assert (tile == 7.25).all() and (mo == 0.5).all(), "the stand-in blend runs nothing"
# ---- the plan pass
for ww, hh in ((0, h), (w, 0), (8193, 1), (1, 8193)):
    refused("size %dx%d" % (ww, hh), plan, P, ww=ww, hh=hh)
refused("moments NULL", plan, P, m=None)
refused("counts NULL", plan, P, c=None)
for te in (0.0, -0.0, -0.05, 1.000001e6, float("nan"), float("inf")):
    refused("targetError %r" % te, plan, P, te=te)
refused("minSamples -1", plan, P, lo=-1)
refused("maxSamples 2048", plan, P, hi=2048)
refused("minSamples over maxSamples", plan, P, lo=9, hi=8)
refused("counts in the moments", plan, P, c=mo.ctypes.data + plane - 4)
refused("variance is the moments", plan, P, v=mo)
refused("total in the moments", plan, P, t=mo.ctypes.data + 8)
refused("variance overlaps the counts", plan, P, c=big.ctypes.data + plane - 4, v=big)
refused("total in the counts", plan, P, t=cnt.ctypes.data + 8)
refused("total in the variance", plan, P, t=var.ctypes.data + plane - 8)
# two rules broken at once: the one that is checked first is the one reported
def order(expect, **kw):
    rc = plan(**kw)
    msg = lib.tptGetLastError().decode()
    assert rc != 0 and msg == P + ": " + expect, (expect, sorted(kw), rc, msg)
    print("order:", sorted(kw), "--", expect)
order("deviceMoments and deviceSampleCounts are required", c=None, te=0.0)
order("targetError must lie in (0, 1e6]", te=0.0, lo=-1)
order("0 <= minSamples <= maxSamples <= 2047 expected", lo=-1, v=mo)
order("an output overlaps deviceMoments", c=mo.ctypes.data + plane - 4, t=var.ctypes.data + 8)  # (the input's pairs before the outputs')
order("an output overlaps deviceMoments", v=big, c=big.ctypes.data + plane - 4, t=mo.ctypes.data + 8)  # (... the last of them too)
assert emu.hostemuAdaptivePlans() == 0, "a refused plan reached the launcher"
for kw in (dict(), dict(v=None), dict(t=None), dict(v=None, t=None), dict(te=1e6), dict(te=1e-30), dict(lo=0, hi=0), dict(lo=2047, hi=2047),
           dict(ww=1, hh=1), dict(v=big, c=big.ctypes.data + plane)):
    assert plan(**kw) == 0, (kw, lib.tptGetLastError().decode())
    print("accepted:", sorted(kw))
assert emu.hostemuAdaptivePlans() == 10
tpt.synchronize()
assert (mo == 0.5).all() and (cnt == 4).all() and (var == -2.0).all() and tot[0] == -9, "a refused plan wrote (the stand-in runs nothing)"
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_through_the_host_runtime():
    out = run_refusals(REFUSALS, "libtpt_hostemu_adaptive.so", ["hostemu_adaptive.cpp"])
    assert out.count("refused:") == 2 + 16 + 5 + 4 + 2 + 6 + 3 + 6, out
    assert out.count("accepted:") == 2 + 10, out
    assert out.count("order:") == 5, out
    D, P = "tptDrawDeviceAdaptive: ", "tptAdaptiveSamplesDevice: "
    assert refusal_messages(out) == {
        "tpt: not initialised (call tptInitialize / InitializeTest first)": 2,
        D + "call tptUpdate (UpdateTest) at this size first": 2,
        D + "bad arguments (deviceTile, deviceMoments, deviceSampleCounts, size)": 3,
        D + "deviceMoments overlaps the tile or a plane": 4,
        D + "frames of at most 8192 x 8192": 1,
        D + "needs per-pixel seeds (tptSetSeedMode(1)); row-serial sample counts are not supported": 1,
        D + "needs the recursive fold (tptSetFoldMode(0))": 1,
        D + "needs the path-queue kernel (tptSetKernelVariant(0, 3, ..))": 2,
        D + "not with row sharding or a communicator (sharded sample counts are not supported)": 2,
        D + "not with a tile mirror (tptSetTileMirror)": 1,
        D + "deviceSampleCounts overlaps the tile, the moments or a plane": 4,
        P + "w and h must lie in 1..8192": 4,
        P + "deviceMoments and deviceSampleCounts are required": 2,
        P + "targetError must lie in (0, 1e6]": 6,
        P + "0 <= minSamples <= maxSamples <= 2047 expected": 3,
        P + "an output overlaps deviceMoments": 3,
        P + "two outputs overlap": 3,
    }


def test_a_build_without_the_plan_launcher_refuses():
    refused_without_its_launcher('''
mo, cnt = np.full((8, 16, 4), 0.5, np.float32), np.full((8, 16), 4, np.int32)
rc = lib.tptAdaptiveSamplesDevice(16, 8, mo.ctypes.data, 0.05, 0, 64, cnt.ctypes.data, None, None)
tpt.synchronize()
assert (cnt == 4).all()
''', "tptAdaptiveSamplesDevice: this build has no adaptive plan kernel")
