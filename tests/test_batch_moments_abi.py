"""tptDrawDeviceBatchMoments without a GPU: the declaration and the words of its statement; the binding, the export and the binding's
argument checks; the gfx950 code of the fold kernel (tptFoldBatchKernel) in the shipped library; and the host side through the runtime
compiled against tests/hostemu -- every refusal and the launch plan of accepted calls with tests/hostemu_batch_moments.cpp's counting
launchers (they run nothing and show what they were handed), and the data flow across chunk seams, calls and a growing staging with
tests/hostemu_batch_moments_flow.cpp's stand-ins, held byte for byte against the statement in numpy (tests/batch_moments_lib.py)."""
import os
import re
import subprocess
import sys

import pytest

from isa_lib import code_object, count, exported_symbols, header_params, no_library, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import FOLD
from oracle_lib import ROOT

NAME = "tptDrawDeviceBatchMoments"
# DESIGN.md 3.17 records these from the code object's notes
FOLD_VGPRS, FOLD_SGPRS = 30, 41
# the launchers tests/hostemu/hostemu_kernels.cpp defines and the counting / stand-in files take over (the linker's --wrap, per symbol)
TRACE_QUEUE = "_Z19tptLaunchTraceQueueRKN3tpt10KernelArgsEbimP12ihipStream_t"
TRACE = "_Z14tptLaunchTraceRKN3tpt10KernelArgsEiibimP12ihipStream_t"
RESOLVE = "_Z16tptLaunchResolvePfPKN3tpt2f4EifS_PyS4_PKyP12ihipStream_t"
RESOLVE_BATCH = "_Z21tptLaunchResolveBatchPfPKN3tpt2f4EiiiRK12tptLerpTableS_PyS7_P12ihipStream_t"


# ---------------------------------------------------------------- the declaration, the binding, the export
def test_header_declares_the_entry_point_and_states_it():
    assert header_params(NAME) == ["float time", "int firstFrame", "int nFrames", "int screenWidth", "int screenHeight", "float* deviceTile",
                                   "float* deviceMoments", "float* deviceAlbedo", "float* deviceNormalDepth", "unsigned testFlags"]
    text = open(os.path.join(ROOT, "include", "tpt_hip.h")).read()
    doc = text[text.index("Progressive frames with averaged guides"):text.index("TPT_API int " + NAME)]
    for words in ("byte\n * for byte, and ray for ray", "tptDrawDeviceMoments(time, firstFrame + j, w, h, deviceTile, A_j, ND_j, deviceMoments, testFlags)",
                  "deviceAlbedo      = deviceAlbedo      * lerp_j + A_j  * (1 - lerp_j)", "deviceNormalDepth = deviceNormalDepth * lerp_j + ND_j * (1 - lerp_j)",
                  "all four channels", "binary32", "no FMA", "1 - lerp_j formed in binary32", "alpha", "untouched", "finite", "tptDenoiseDeviceVariance",
                  "exactly once", "Asynchronous", "4096 MiB", "never refused", "Refused", "nFrames < 1", "firstFrame < 0", "TPT_FLAG_ANIMATE",
                  "sharing a byte", "more lights"):
        assert words in doc, words
    # the filter's advice to a progressive caller now names the call
    advice = text[text.index("a progressive\n * caller averages the albedo"):]
    assert NAME in advice[:400]


def test_binding_and_export():
    import ctypes as C
    from toypathtracer_amd import api
    assert NAME in api.C_ABI_SYMBOLS and callable(api.draw_device_batch_moments)
    lib = api.load_library()
    assert lib.tptDrawDeviceBatchMoments.argtypes == [C.c_float] + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_uint]
    assert re.search(r"\bT %s\b" % NAME, exported_symbols(api.library_path()))


@pytest.mark.parametrize("args", [
    dict(w=0), dict(h=-3), dict(w=8.0), dict(n=0), dict(n=-1), dict(n=2.0), dict(n=True), dict(first=-1), dict(first=1.0), dict(first=None),
    dict(first=2 ** 31 - 1), dict(first=2 ** 31 - 2, n=3), dict(tile=0), dict(tile=None), dict(mo=None), dict(mo=0), dict(mo=1.5),
    dict(albedo=-16), dict(albedo="x"), dict(nd=2.0), dict(nd=True),
], ids=lambda a: ",".join("%s=%r" % kv for kv in a.items()))
def test_binding_checks_arguments_before_the_library(monkeypatch, args):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(first=0, n=2, w=16, h=8, tile=4096, mo=8192, albedo=None, nd=None)
    a.update(args)
    with pytest.raises(ValueError):
        api.draw_device_batch_moments(0.0, a["first"], a["n"], a["w"], a["h"], a["tile"], a["mo"], 2, albedo_ptr=a["albedo"], normal_depth_ptr=a["nd"])


# ---------------------------------------------------------------- the shipped gfx950 code
def test_fold_kernel_in_the_code_object(code_object):  # noqa: F811
    bodies, meta = code_object
    assert FOLD in meta and FOLD in bodies, "the fold kernel is missing from the shipped code object"
    body, m = bodies[FOLD], meta[FOLD]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] == 0 and m["agpr_count"] == 0, m
    assert count(body, r"flat_") == 0 and count(body, r"buffer_") == 0 and count(body, r"scratch_") == 0 and count(body, r"ds_") == 0
    # every access of a plane is 16 bytes (12 where the tile's alpha and the moments' .w are neither blended nor written)
    loads = [ins[0] for ins in body if ins and ins[0].startswith("global_load")]
    stores = [ins[0] for ins in body if ins and ins[0].startswith("global_store")]
    assert loads and stores
    assert set(loads) <= {"global_load_dwordx4", "global_load_dwordx3"}, loads
    assert set(stores) <= {"global_store_dwordx4", "global_store_dwordx3"}, stores
    # the four-channel planes do move 16 bytes: an unrolled group of four staged loads and the running value, and its store
    assert loads.count("global_load_dwordx4") >= 5 and stores.count("global_store_dwordx4") >= 1
    # the ray counts: scalar loads, and the one atomic on the total
    assert count(body, r"global_atomic_add_x2") == 1 and count(body, r"global_atomic") == 1
    assert count(body, r"s_setprio") >= 1
    assert (m["vgpr_count"], m["sgpr_count"]) == (FOLD_VGPRS, FOLD_SGPRS), m
    assert m["vgpr_count"] <= 32, "beside four 120-VGPR trace waves a SIMD has 32 registers a lane left"
    assert m["max_flat_workgroup_size"] == 256 and m["wavefront_size"] == 64


def test_exactly_one_new_kernel_and_every_count_unchanged(code_object):  # noqa: F811
    """(every other family: tests/test_isa_contract.py holds the library to exactly tests/kernel_manifest.py)"""
    _, meta = code_object
    assert [n for n in meta if "Fold" in n] == [FOLD]


# ---------------------------------------------------------------- the host side, through the emulated runtime
def run_script(script, lib, source, wraps, env=None):
    """`script` (given ROOT as argv[1]) against the host runtime built for tests/hostemu with tests/`source` beside the emulated kernels,
    whose launchers `wraps` that file takes over; under the lazy schedule; it must end with "ok".  Returns its output."""
    from test_host_logic import build
    path = build(lib, ["-Wl,--wrap=" + s for s in wraps] + [os.path.join(ROOT, "tests", source)])
    e = dict(os.environ, TPT_LIB=path, HOSTEMU_POLICY="lazy", **(env or {}))
    e.pop("TPT_LIB_DIR", None)
    p = subprocess.run([sys.executable, "-c", script, ROOT], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.rstrip().endswith("ok"), out[-3000:]
    return out


COMMON = r'''
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
so = C.CDLL(os.environ["TPT_LIB"])
F = "tptDrawDeviceBatchMoments"
PROGRESSIVE = 2
ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
def reset():
    tpt.set_seed_mode(1); tpt.set_fold_mode(0); tpt.set_kernel_variant(0, 3, -1); tpt.set_row_shard(0, 1, 0); tpt.set_samples_per_pixel(4)
    tpt.set_frame_overlap(16)
def msg():
    return lib.tptGetLastError().decode()
'''

PLAN = COMMON + r'''
w, h = 16, 8
plane = w * h * 16
SENTINELS = (7.25, 0.5, 0.25, 3.0)
tile, mo, alb, nd = (np.full((h, w, 4), v, np.float32) for v in SENTINELS)
big = np.zeros((2, h, w, 4), np.float32)
def call(first=0, n=3, ww=w, hh=h, tl=tile, m=mo, a=alb, d=nd, flags=PROGRESSIVE):
    return lib.tptDrawDeviceBatchMoments(0.0, first, n, ww, hh, ptr(tl), ptr(m), ptr(a), ptr(d), flags)
def counts():
    c = (C.c_longlong * 3)(); so.hostemuBmCounts(c); return list(c)
def trace(i):
    v = (C.c_longlong * 13)(); so.hostemuBmTrace(i, v)
    return dict(zip("frames first colour moments albedo nd aov_plane frame_plane cams centres ray_counter ray_stride queue".split(), v))
def fold(i):
    v, l = (C.c_longlong * 12)(), (C.c_float * 32)(); so.hostemuBmFold(i, v, l)
    d = dict(zip("tile moments albedo nd s_colour s_moments s_albedo s_nd pixels frames frame_rays total_rays".split(), v))
    d["lerp"] = np.float32(list(l)); return d
def scene_desc():
    s, cam = np.zeros(46 * 5, np.float32), np.zeros(22, np.float32)
    lib.tptGetSceneDesc(s.ctypes.data, None, cam.ctypes.data, None, None)
    return s.tobytes() + cam.tobytes()
state = None
def refused(what, expect=F, **kw):
    rc = call(**kw)
    assert rc != 0 and expect in msg(), (what, rc, msg())
    assert counts() == [0, 0, 0], (what, "something was enqueued", counts())
    assert state is None or scene_desc() == state, (what, "the camera or the spheres changed")
    print("refused:", what, "--", msg())
def update(ww, hh):
    global state
    tpt.UpdateTest(0.0, 0, ww, hh, PROGRESSIVE)
    state = scene_desc()
refused("no context", "not initialised")
tpt.InitializeTest(); reset()
refused("before any tptUpdate")
update(w, h)
# ---- what tptDrawDeviceMoments refuses
refused("tile NULL", tl=None)
refused("moments NULL", m=None)
refused("width 0", ww=0)
refused("no tptUpdate at this size", hh=h + 1)
update(8200, 8)
refused("wider than 8192", ww=8200, hh=8)
update(w, h)
tpt.set_row_shard(8, 2, 0); refused("row sharding"); reset()
tpt.comm_init_loopback(2, 8); refused("communicator"); tpt.comm_destroy(); reset()
mirror = np.zeros((h, w, 4), np.float32)
tpt.set_tile_mirror(mirror.ctypes.data); refused("tile mirror"); tpt.set_tile_mirror(None)
tpt.set_seed_mode(0); refused("row-serial seeds"); reset()
tpt.set_fold_mode(1); refused("forward fold"); reset()
for hs, persist in ((0, 1), (1, 3)):
    tpt.set_kernel_variant(hs, persist, -1); refused("variant %d/%d" % (hs, persist))
reset()
tpt.set_samples_per_pixel(2048); refused("2048 spp"); reset()
# ---- its own
refused("0 frames", n=0)
refused("-1 frames", n=-1)
refused("firstFrame -1", first=-1)
refused("a last frame past 2^31 - 1", first=2 ** 31 - 2, n=3)
refused("TPT_FLAG_ANIMATE", flags=3)
refused("TPT_FLAG_ANIMATE alone", flags=1)
refused("an unknown flag bit", flags=PROGRESSIVE | 8)
refused("moments is the tile", m=tile)
refused("albedo is the normal / depth", a=nd)
refused("albedo is the tile", a=tile)
refused("normal / depth is the moments", d=mo)
refused("moments start in the tile's last pixel", m=tile.ctypes.data + plane - 16)
refused("albedo ends in the normal / depth's first pixel", a=big, d=big.ctypes.data + plane - 4)
import lights_lib
tpt.set_scene(*lights_lib.stress_with_lights(4096, 64, 3072)); tpt.UpdateTest(0.0, 0, w, h, PROGRESSIVE)
state = None  # (scene_desc reads the built-in scene's 46 spheres)
refused("3072 lights"); assert "3072 emissive spheres" in msg() and "at most 2864" in msg(), msg()
tpt.set_scene(None); update(w, h)
tpt.synchronize()
for p, v in zip((tile, mo, alb, nd), SENTINELS):
    assert (p == v).all(), "a refused call wrote"
assert (big == 0).all()

# ---- the launch plan of accepted calls
def lerps(first, n, flags=PROGRESSIVE):
    return np.float32([np.float32(f) / np.float32(f + 1) if flags & PROGRESSIVE else 0 for f in range(first, first + n)])
def accepted(n, first=0, a=alb, d=nd, flags=PROGRESSIVE, per_launch=32):
    so.hostemuBmReset()
    assert call(first=first, n=n, a=a, d=d, flags=flags) == 0, msg()
    chunks = [min(per_launch, n - f) for f in range(0, n, per_launch)]
    assert counts() == [len(chunks), len(chunks), 0], (counts(), "one fold behind each trace launch, and no per-frame resolve")
    at = first
    recs = []
    for i, c in enumerate(chunks):
        t, f = trace(i), fold(i)
        assert (t["frames"], t["first"], t["queue"]) == (c, at, 1), t
        assert (f["frames"], f["pixels"]) == (c, w * h), f
        assert (f["tile"], f["moments"], f["albedo"], f["nd"]) == (ptr(tile), ptr(mo), ptr(a) or 0, ptr(d) or 0), "the caller's planes, NULL as NULL"
        assert (f["s_colour"], f["s_moments"], f["s_albedo"], f["s_nd"]) == (t["colour"], t["moments"], t["albedo"], t["nd"]), "the fold reads what the launch wrote"
        assert f["s_colour"] and f["s_moments"] and bool(f["s_albedo"]) == (a is not None) and bool(f["s_nd"]) == (d is not None)
        assert t["frame_plane"] == w * h and f["lerp"][:c].tobytes() == lerps(at, c, flags).tobytes() and not f["lerp"][c:].any(), f["lerp"]
        recs.append((t, f))
        at += c
    tpt.synchronize()
    return recs
recs = accepted(70)
for t, f in recs:
    assert t["cams"] and t["centres"] and t["aov_plane"] == w * h and t["ray_stride"] == 1, "the camera-clip launch: both tables, a plane and a ray counter per frame"
    assert f["frame_rays"] == t["ray_counter"] and f["total_rays"] and f["total_rays"] != f["frame_rays"]
    assert t["nd"] - t["albedo"] == t["frames"] * plane, "normal / depth behind the albedo planes of the launch's frames"
# the halves of the staging: launches 0 and 2 share one, launch 1 has the other, a largest launch's planes further on
assert recs[0][0]["albedo"] == recs[2][0]["albedo"] and recs[0][0]["moments"] == recs[2][0]["moments"]
assert abs(recs[1][0]["albedo"] - recs[0][0]["albedo"]) == 2 * 32 * plane and abs(recs[1][0]["moments"] - recs[0][0]["moments"]) >= 32 * plane
accepted(1); accepted(33, first=5); accepted(3, flags=0)
r = accepted(33, a=None)
assert all(t["nd"] - 0 and not t["albedo"] for t, _ in r)
assert abs(r[1][0]["nd"] - r[0][0]["nd"]) == 2 * 32 * plane, "the staging never shrinks: the halves stay where the 70-frame call put them"
accepted(33, d=None); accepted(33, a=None, d=None)
# a scene of 4 spheres: a frame per launch, the single-frame kernel (no tables, the kernel counts its rays itself)
s, m, _, _ = tpt.GetSceneDesc()
tpt.set_scene(s[:4].copy(), m[:4].copy()); tpt.UpdateTest(0.0, 0, w, h, PROGRESSIVE)
for t, f in accepted(70, per_launch=1):
    assert not t["cams"] and not t["centres"] and t["aov_plane"] == 0 and f["frame_rays"] == 0 and t["ray_counter"] == f["total_rays"]
tpt.set_scene(None); tpt.UpdateTest(0.0, 0, w, h, PROGRESSIVE)
# frames per launch: the most whose staging stays within 4096 MiB
m = so.hostemuBmFramesPerLaunch
assert [m(640, 360, 4), m(1280, 720, 4), m(3840, 2160, 4), m(3840, 2160, 2)] == [32, 32, 8, 16]
assert [m(8192, 4096, 4), m(8192, 4096, 3), m(8192, 4096, 2), m(8192, 8192, 4), m(8192, 8192, 2)] == [2, 2, 4, 1, 2]
for ww, hh, planes in ((8192, 4096, 4), (4096, 4096, 3), (2048, 2048, 4), (3840, 2160, 4)):
    k = m(ww, hh, planes)
    assert k * planes * ww * hh * 16 <= 4096 << 20 and (k == 32 or (k + 1) * planes * ww * hh * 16 > 4096 << 20), (ww, hh, planes, k)
# 2048 x 1024 with both guides is 128 MiB a frame, 32 frames exactly the limit; 2048 x 1032 takes 31 (the arithmetic alone: the emulated
# device touches every byte it allocates, and such a call stages gigabytes)
assert m(2048, 1024, 4) == 32 and m(2048, 1032, 4) == 31
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_and_the_launch_plan_through_the_host_runtime():
    out = run_script(PLAN, "libtpt_hostemu_batch_moments.so", "hostemu_batch_moments.cpp", [TRACE_QUEUE, TRACE, RESOLVE, RESOLVE_BATCH])
    assert out.count("refused:") == 2 + 5 + 3 + 5 + 4 + 3 + 6 + 1, out


NO_LAUNCHER = COMMON + r'''
w, h = 16, 8
planes = [np.full((h, w, 4), 1.5, np.float32) for _ in range(4)]
tpt.InitializeTest(); reset()
tpt.UpdateTest(0.0, 0, w, h, PROGRESSIVE)
rc = lib.tptDrawDeviceBatchMoments(0.0, 0, 3, w, h, *[p.ctypes.data for p in planes], PROGRESSIVE)
assert rc != 0 and F in msg() and "no fold kernel" in msg(), (rc, msg())
tpt.synchronize()
assert all((p == 1.5).all() for p in planes)
tpt.ShutdownTest()
print("ok")
'''


def test_a_runtime_without_the_fold_launcher_loads_and_refuses_by_name():
    run_refusals(NO_LAUNCHER)


FLOW = COMMON + r'''
from batch_moments_lib import fold_frames
w, h = 12, 5
n_pix = w * h
def stand_in(frame, plane):
    i = np.arange(n_pix, dtype=np.int64)[:, None]
    ch = np.arange(4, dtype=np.int64)[None, :]
    return (((frame * 131 + i * 7 + plane * 17 + ch * 3) % 1009).astype(np.float32) / np.float32(64) + np.float32(0.5)).reshape(h, w, 4)
def frames(first, n):
    return [tuple(stand_in(first + j, k) for k in range(4)) for j in range(n)]
def rays(first, n):
    return sum(1000 + 37 * f for f in range(first, first + n))
def start():
    rng = np.random.default_rng(11)
    return [rng.random((h, w, 4), dtype=np.float32) * np.float32(4) - np.float32(1) for _ in range(4)]
def run(calls, flags=PROGRESSIVE, guides=(True, True), first=0):
    planes = start()
    given = [planes[0], planes[1], planes[2] if guides[0] else None, planes[3] if guides[1] else None]
    before = tpt.ray_counter_read()
    at = first
    for n in calls:
        assert lib.tptDrawDeviceBatchMoments(0.0, at, n, w, h, *[ptr(p) for p in given], flags) == 0, msg()
        tpt.synchronize()
        at += n
    return planes, tpt.ray_counter_read() - before
def want(n, flags=PROGRESSIVE, guides=(True, True), first=0):
    planes = start()
    fold_frames(planes[0], planes[1], planes[2] if guides[0] else None, planes[3] if guides[1] else None, frames(first, n), first, flags)
    return planes
def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
tpt.InitializeTest(); reset()
tpt.UpdateTest(0.0, 0, w, h, PROGRESSIVE)
mutant = os.environ.get("HOSTEMU_FOLD_MUTANT")
one, r = run([70])
if mutant:
    assert not same(one, want(70)), "the mutant fold (%s) left the bytes as they were" % mutant
    assert one[0][..., 3].tobytes() == start()[0][..., 3].tobytes()
    tpt.ShutdownTest(); print("ok"); sys.exit(0)
assert same(one, want(70)) and r == rays(0, 70), "70 frames in one call against the numpy recurrence"
assert one[0][..., 3].tobytes() == start()[0][..., 3].tobytes() and one[1][..., 3].tobytes() == start()[1][..., 3].tobytes(), "the tile's alpha, the moments' .w"
tpt.ShutdownTest(); tpt.InitializeTest(); reset(); tpt.UpdateTest(0.0, 0, w, h, PROGRESSIVE)   # (a fresh context: the staging starts small and grows)
split, r = run([20, 13, 37])
assert same(split, one) and r == rays(0, 70), "20 + 13 + 37 frames, the staging growing, against one call"
for flags, guides, first, n in ((0, (True, True), 0, 33), (PROGRESSIVE, (False, True), 5, 33), (PROGRESSIVE, (True, False), 0, 65),
                                (PROGRESSIVE, (False, False), 3, 34), (PROGRESSIVE, (True, True), 7, 1)):
    got, r = run([n], flags, guides, first)
    assert same(got, want(n, flags, guides, first)) and r == rays(first, n), (flags, guides, first, n)
# the frame-by-frame path: a scene of 4 spheres
s, m, _, _ = tpt.GetSceneDesc()
tpt.set_scene(s[:4].copy(), m[:4].copy()); tpt.UpdateTest(0.0, 0, w, h, PROGRESSIVE)
got, r = run([5, 2])
assert same(got, want(7)) and r == rays(0, 7), "a frame per launch"
tpt.ShutdownTest()
print("ok")
'''


def run_flow(mutant=None):
    return run_script(FLOW, "libtpt_hostemu_batch_moments_flow.so", "hostemu_batch_moments_flow.cpp", [TRACE_QUEUE],
                      {"HOSTEMU_FOLD_MUTANT": mutant} if mutant else None)


def test_data_flow_against_the_numpy_recurrence():
    """stand-ins that run (tests/hostemu_batch_moments_flow.cpp): every frame's planes depend on its frame number, so a fold that read a
    stale or clobbered staging plane, the other half, or another frame's lerp factor changes the bytes"""
    run_flow()


@pytest.mark.parametrize("mutant", ["slot", "lerp"])
def test_a_fold_that_reads_the_wrong_slot_or_lerp_entry_changes_bytes(mutant):
    """the harness's own sanity: the stand-in fold made to read staged frame j + 1 for frame j, or the lerp table one entry late"""
    run_flow(mutant)
