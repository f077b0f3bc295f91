"""tptTraceRaysDevice without a GPU: the declaration, binding and export; the binding's argument checks; the struct's layout; the code
object's kernel set (no kernel of its own); and, through the host runtime compiled against tests/hostemu with tests/hostemu_rays.cpp
as the launcher, every refusal (no launch, no byte written) and the accepted calls under the eager, lazy and random schedules, held
byte for byte against tests/rays_checker.c."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from isa_lib import code_object, exported_symbols, header, header_params, no_library, refusal_messages, run_refusals  # noqa: F401  (code_object: a fixture)
from kernel_manifest import TRACE, family
from oracle_lib import ROOT

NAME = "tptTraceRaysDevice"
CTYPES_OF = {"int": C.c_int, "unsigned": C.c_uint}


def struct_fields():
    body = re.search(r"typedef\s+struct\s+tptTraceRaysArgs\s*\{(.*?)\}\s*tptTraceRaysArgs\s*;", header(), flags=re.S)
    assert body, "tptTraceRaysArgs is not declared in include/tpt_hip.h"
    fields = []
    for decl in body.group(1).split(";"):
        decl = " ".join(decl.split())
        if decl:
            m = re.match(r"(.*?[\s*])(\w+)$", decl)
            fields.append((m.group(2), m.group(1).strip()))
    return fields


def test_header_declares_the_entry_point_and_states_it():
    from toypathtracer_amd import api
    assert header_params(NAME) == ["const tptTraceRaysArgs* args"]
    fields = struct_fields()
    assert fields == [("nRays", "int"), ("flags", "unsigned"), ("deviceRays", "const float*"), ("deviceRadiance", "float*"),
                      ("deviceHits", "float*"), ("deviceRayCount", "unsigned long long*")]
    assert [n for n, _ in fields] == [n for n, _ in api.TraceRaysArgs._fields_]
    for (name, ctype), (_, mirror) in zip(fields, api.TraceRaysArgs._fields_):
        assert mirror is (C.c_void_p if ctype.endswith("*") else CTYPES_OF[ctype]), (name, ctype, mirror)
    text = open(os.path.join(ROOT, "include", "tpt_hip.h")).read()
    doc = text[text.index("THE CALLER'S RAYS"):text.index("typedef struct tptTraceRaysArgs")]
    for words in ("NOT normalised", "bits(-1)", "0.0f + Trace", "shadow rays included", "k = 1", "tptRayCounterRead", "Refused",
                  "TPT_MAX_LIGHTS", "Maths.cpp:165-202", "never leaves 0"):
        assert words in doc, words


def test_struct_layout_matches_the_ctypes_mirror(tmp_path):
    from toypathtracer_amd import api
    names = [n for n, _ in api.TraceRaysArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tpt_hip.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(tptTraceRaysArgs));\n'
                   + "".join('    printf("%%zu\\n", offsetof(tptTraceRaysArgs, %s));\n' % n for n in names) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert got == [C.sizeof(api.TraceRaysArgs)] + [getattr(api.TraceRaysArgs, n).offset for n in names]
    assert got[0] == 40


def test_binding_and_export():
    from toypathtracer_amd import api
    lib = api.load_library()
    assert NAME in api.C_ABI_SYMBOLS and hasattr(lib, NAME) and callable(api.trace_rays_device)
    assert re.search(r"\bT %s\b" % NAME, exported_symbols(api.library_path()))
    assert re.search(r"^\s*tpt\*;", open(os.path.join(ROOT, "toypathtracer_amd", "csrc", "exports.map")).read(), flags=re.M)


@pytest.mark.parametrize("args", [
    dict(n=0), dict(n=-1), dict(n=16777217), dict(n=2.0), dict(n=True), dict(n=None), dict(rays=0), dict(rays=None), dict(rays=-8),
    dict(rays=1.5), dict(rays="r"), dict(radiance=None, hits=None), dict(radiance=0, hits=0), dict(radiance=1.5), dict(hits=-1),
    dict(hits="h"), dict(count=-1), dict(count=2.5), dict(count=True),
], ids=lambda a: ",".join("%s=%.20r" % kv for kv in a.items()))
def test_binding_checks_arguments_before_the_library(monkeypatch, args):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(n=16, rays=4096, radiance=8192, hits=12288, count=None)
    a.update(args)
    with pytest.raises(ValueError):
        api.trace_rays_device(a["n"], a["rays"], a["radiance"], a["hits"], a["count"])


def test_the_code_object_has_no_kernel_of_its_own(code_object):  # noqa: F811
    """the ray source is a mode of the lane-refill kernel: its eight instantiations and nothing named after rays (the whole set:
    tests/test_isa_contract.py holds the library to exactly tests/kernel_manifest.py)"""
    bodies, meta = code_object
    assert sorted(n for n in meta if "tptTraceKernel" in n) == sorted(family(TRACE))
    assert not [n for n in meta if re.search(r"rays?", n, flags=re.I) and "tptTrace" not in n and "Array" not in n]
    for name in family(TRACE):
        # a ray's records: 16-byte loads and stores (the colour store, the radiance store, the two hit records)
        ops = [ins[0] for ins in bodies[name] if ins]
        assert sum(1 for o in ops if o == "global_store_dwordx4") >= 4, name


SCRIPT = r'''
import ctypes as C, os, sys, tempfile
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from toypathtracer_amd import api as tpt
from toypathtracer_amd.scenes import cloud_scene
from oracle_lib import FLAG_PROGRESSIVE, SEED_PER_PIXEL, Oracle
from common import oracle_frames
import rays_lib
from rays_lib import RaysChecker, all_rays, catalogue, scene_camera
REFUSALS = sys.argv[2] == "refusals"
lib = tpt.load_library()
so = C.CDLL(tpt.library_path())
checker = RaysChecker(tempfile.mkdtemp(prefix="rays_abi_"))
ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
def msg(): return lib.tptGetLastError().decode()
def ops():
    st = (C.c_longlong * 2)(); so.hostemu_stats(st); return st[0]
def raw(n, rays, rad, hits, count, flags=0):
    a = tpt.TraceRaysArgs(nRays=n, flags=flags, deviceRays=ptr(rays), deviceRadiance=ptr(rad), deviceHits=ptr(hits), deviceRayCount=ptr(count))
    return lib.tptTraceRaysDevice(C.byref(a))
W, H = 16, 8
N = 100
rays0 = checker.camera_rays(Oracle.get().default_camera(40, 25), 40, 25)[:N].copy()
big = np.full((4 * N + 8, 8), np.nan, np.float32)
count = np.full(4, 7, np.uint64)
def fresh():
    return rays0.copy(), np.full((N, 4), np.nan, np.float32), np.full((N, 8), np.nan, np.float32)
if REFUSALS:
    def refused(what, **kw):
        r, rad, hits = fresh()
        a = dict(n=N, rays=r, rad=rad, hits=hits, count=count, flags=0)
        a.update(kw)
        rc = raw(a["n"], a["rays"], a["rad"], a["hits"], a["count"], a["flags"])
        assert rc != 0 and "tptTraceRaysDevice" in msg(), (what, rc, msg())
        print("refused:", what, "--", msg())
        return rad, hits
    rc = raw(N, *fresh(), count)
    assert rc != 0 and "not initialised" in msg(), msg()
    print("refused: no context --", msg())
    tpt.InitializeTest()
    refused("before any tptUpdate")
    tpt.UpdateTest(0.0, 0, W, H, 0)
    tpt.synchronize()
    ops0 = ops()
    kept = []
    assert lib.tptTraceRaysDevice(None) != 0 and "tptTraceRaysDevice" in msg()
    print("refused: args NULL --", msg())
    for n in (0, -1, 16777217, -(1 << 31)):
        kept.append(refused("nRays %d" % n, n=n))
    for flags in (1, 2, 0x80000000):
        kept.append(refused("flags %#x" % flags, flags=flags))
    kept.append(refused("deviceRays NULL", rays=None))
    kept.append(refused("both outputs NULL", rad=None, hits=None))
    b = big.ctypes.data
    for what, kw in (("radiance is the rays", dict(rays=b, rad=b)), ("hits are the rays", dict(rays=b, hits=b)),
                     ("radiance's head in the rays' tail", dict(rays=b, rad=b + 32 * N - 4)),
                     ("the rays' head in the radiance's tail", dict(rad=b, rays=b + 16 * N - 16)),
                     ("hits' head in the rays' tail", dict(rays=b, hits=b + 32 * N - 32)),
                     ("the rays' head in the hits' tail", dict(hits=b, rays=b + 32 * N - 4)),
                     ("radiance in the hits", dict(hits=b, rad=b + 32 * N - 16)),
                     ("hits in the radiance", dict(rad=b, hits=b + 16 * N - 4)),
                     ("the counter in the rays", dict(rays=b, count=b + 32 * N - 8)),
                     ("the counter in the radiance", dict(rad=b, count=b + 8)),
                     ("the counter in the hits", dict(hits=b, count=b + 32 * N - 8))):
        kept.append(refused("overlap: " + what, **kw))
    # two rules broken at once: the one that is checked first is the one reported
    def order(expect, **kw):
        r, rad, hits = fresh()
        a = dict(n=N, rays=r, rad=rad, hits=hits, count=count, flags=0)
        a.update(kw)
        rc = raw(a["n"], a["rays"], a["rad"], a["hits"], a["count"], a["flags"])
        assert rc != 0 and msg() == "tptTraceRaysDevice: " + expect, (expect, kw, rc, msg())
        print("order:", sorted(kw), "--", expect)
        kept.append((rad, hits))
    order("nRays must lie in 1..16777216", n=0, flags=1)
    order("flags must be 0", flags=1, rays=None)
    order("deviceRays is required", rays=None, rad=None, hits=None)
    order("deviceRadiance or deviceHits is required", rad=None, hits=None, count=b)
    order("an output overlaps deviceRays", rays=b, rad=b, hits=b + 8)
    order("an output overlaps deviceRays", rays=b, rad=b + 32 * N, hits=b + 48 * N - 4, count=b + 8)  # (the counter is the last pair looked at)
    order("two outputs overlap", rays=b, rad=b + 32 * N, hits=b + 48 * N - 4, count=b + 40 * N)
    # what a scene can do
    s, m = cloud_scene(3100, lights=3073)
    tpt.set_scene(s, m)
    tpt.UpdateTest(0.0, 0, W, H, 0)
    assert len(tpt.GetSceneDesc()[3]) == 3073
    kept.append(refused("3073 emissive spheres"))
    order("two outputs overlap", rad=b, hits=b + 16 * N - 4)  # (the buffers before the scene)
    tpt.set_kernel_variant(2, 1, 1)
    tpt.UpdateTest(0.0, 0, W, H, 0)
    order("too many emissive spheres for the LDS light table (3072 at most)")  # (the lights before the LDS fit)
    tpt.set_kernel_variant(0, 3, -1)
    s, m = cloud_scene(3000)
    tpt.set_scene(s, m)
    tpt.set_kernel_variant(2, 1, 1)  # flat, and staged in LDS whatever its size: 3000 x 68 B
    tpt.UpdateTest(0.0, 0, W, H, 0)
    kept.append(refused("a scene whose LDS does not fit"))
    tpt.set_kernel_variant(0, 3, -1)
    tpt.set_scene(None, None)
    tpt.UpdateTest(0.0, 0, W, H, 0)
    tpt.synchronize()
    assert so.hostemuRayLaunches() == 0, "a refused call reached the launcher"
    for rad, hits in kept:
        assert np.isnan(rad).all() and np.isnan(hits).all(), "a refused call wrote an output"
    assert np.isnan(big).all() and (count == 7).all()
    # accepted at the limits of what is refused: rays | radiance | hits | counter, each starting where the one before ends
    big[:N] = rays0
    big[N + N // 2 + N:] = 0  # (the counter's word)
    assert raw(N, b, b + 32 * N, b + 48 * N, b + 80 * N) == 0, msg()
    tpt.synchronize()
    s, m = tpt.GetSceneDesc()[:2]
    total, wrad, whit = checker.trace(s, m, rays0)
    assert big[:N].tobytes() == rays0.tobytes() and big[N:N + N // 2].tobytes() == wrad.tobytes()
    assert big[N + N // 2:2 * N + N // 2].tobytes() == whit.tobytes() and int(big[2 * N + N // 2:].ravel().view(np.uint64)[0]) == total
    assert so.hostemuRayLaunches() == 1
    print("accepted: buffers that touch")
    tpt.ShutdownTest()
    print("ok")
    sys.exit(0)

# ---------------------------------------------------------------- accepted calls against the checker
tpt.InitializeTest()
def run(rays, radiance=True, hits=True, counted=True, sync=True):
    """-> (radiance, hits, counter word) with a guard row before and after each output"""
    n = len(rays)
    rad = np.full((n + 2, 4), np.nan, np.float32) if radiance else None
    hit = np.full((n + 2, 8), np.nan, np.float32) if hits else None
    cnt = np.array([5, 1000, 5], np.uint64)
    tpt.trace_rays_device(n, ptr(rays), ptr(rad) + 16 if radiance else None, ptr(hit) + 32 if hits else None, ptr(cnt) + 8 if counted else None)
    out = dict(rad=rad, hit=hit, cnt=cnt, n=n, counted=counted)
    if sync:
        tpt.synchronize()
    return out
def check(out, want, what):
    total, wrad, whit = want
    for got, w, name in ((out["rad"], wrad, "radiance"), (out["hit"], whit, "hits")):
        if got is None:
            continue
        assert np.isnan(got[0]).all() and np.isnan(got[-1]).all(), (what, name, "a guard row was written")
        if got[1:-1].tobytes() != w.tobytes():
            bad = np.argwhere(got[1:-1].view(np.uint32) != w.view(np.uint32))
            raise AssertionError("%s: %s: %d words differ, first at %s: %r / %r" % (what, name, len(bad), bad[0], got[1:-1][bad[0][0]], w[bad[0][0]]))
    assert out["cnt"].tolist() == [5, 1000 + (total if out["counted"] else 0), 5], (what, out["cnt"], total)
# the bounce-stack spill grows between the calls of one sequence: in the context's default mode -- the recursive fold (tptSetFoldMode(0))
# with 6 of the 10 stack levels in LDS -- a launch has a spill column per thread (Context::dRayStack), so 64 rays need one workgroup's,
# 4096 rays 64 workgroups'.  Small, large, small again with no wait in between: the growth itself drains the context stream (under the
# lazy schedule nothing else runs the first call before its buffer goes), and every call's records are the checker's.
def stats():
    st = (C.c_longlong * 2)(); so.hostemu_stats(st); return st[0], st[1]
tpt.UpdateTest(0.0, 0, W, H, 0)
s, m = rays_lib.default_scene()
grid = checker.camera_rays(Oracle.get().default_camera(64, 64), 64, 64)
small, large = np.ascontiguousarray(grid[:64]), np.ascontiguousarray(grid[:4096])
first = run(small, sync=False)
ran, frees = stats()
second = run(large, sync=False)
assert stats()[1] == frees + 1, "the spill did not grow"
assert stats()[0] > ran, "the growth did not drain the context stream"
third = run(small, sync=False)
assert stats()[1] == frees + 1, "the spill was replaced again"
tpt.synchronize()
for out, r, what in ((first, small, "before the growth"), (second, large, "the call that grows the spill"), (third, small, "after the growth")):
    check(out, checker.trace(s, m, r), what)
print("accepted: the spill grows between calls")
n_calls = 0
for scene in ("default", "grouped"):
    s, m = rays_lib.SCENES[scene]()
    tpt.set_scene(s, m) if scene != "default" else tpt.set_scene(None, None)
    tpt.UpdateTest(0.0, 0, W, H, 0)
    info = tpt.scene_info()
    assert (info["groups"] > 0) == (scene == "grouped"), info
    rays, where = all_rays(catalogue(checker, s, scene_camera(scene, 40, 25)))
    for light_sampling in (True, False):
        tpt.set_config(light_sampling=light_sampling)
        for fold in (0, 1):
            tpt.set_fold_mode(fold)
            want = {(True, True): checker.trace(s, m, rays, fold=fold, light_sampling=light_sampling),
                    (True, False): checker.trace(s, m, rays, hits=False, fold=fold, light_sampling=light_sampling),
                    (False, True): checker.trace(s, m, rays, radiance=False, fold=fold, light_sampling=light_sampling)}
            assert want[(False, True)][0] == len(rays)
            for hs in (0, 1):
                tpt.set_kernel_variant(hs, 3, -1)
                for (radiance, hits), w in want.items():
                    for counted in (True, False):
                        if not light_sampling and not (radiance and hits and counted):
                            continue  # (the switch is the radiance's: one call per kernel shows it)
                        r0 = tpt.ray_counter_read()
                        check(run(rays, radiance, hits, counted), w, "%s ls=%d fold=%d hs=%d %s%s%s" % (
                            scene, light_sampling, fold, hs, "R" if radiance else "", "H" if hits else "", "C" if counted else ""))
                        assert tpt.ray_counter_read() == r0, "the context's ray counter moved"
                        n_calls += 1
    tpt.set_config()
    tpt.set_fold_mode(0)
    tpt.set_kernel_variant(0, 3, -1)
print("accepted: %d calls equal the checker" % n_calls)

# ray counts around a chunk and a wave, one ray, and more chunks than the emulated machine has waves
tpt.set_scene(None, None)
tpt.UpdateTest(0.0, 0, W, H, 0)
s, m = rays_lib.default_scene()
cam_rays = checker.camera_rays(Oracle.get().default_camera(64, 40), 64, 40)
for n in (1, 63, 64, 65, 255, 256, 257, 2560):
    r = np.ascontiguousarray(cam_rays[:n])
    check(run(r), checker.trace(s, m, r), "n = %d" % n)
print("accepted: the ray counts")

# two calls back to back (the emulation aborts if the second finds the first's counters in use), the second adding to the same word
r = np.ascontiguousarray(cam_rays[:300])
want = checker.trace(s, m, r)
cnt = np.zeros(1, np.uint64)
outs = [np.full((300, 4), np.nan, np.float32) for _ in range(3)]
for o in outs:
    tpt.trace_rays_device(300, ptr(r), ptr(o), None, ptr(cnt))
tpt.synchronize()
assert all(o.tobytes() == want[1].tobytes() for o in outs) and int(cnt[0]) == 3 * want[0]
print("accepted: three calls back to back")

# the scene a call reads is the one staged when it was made, whatever is set and staged behind it
s2, m2 = s.copy(), m.copy()
s2["cy"][1:] += np.float32(0.75)
m2["albedo"][:] = 0.25
want2 = checker.trace(s2, m2, r)
assert want2[1].tobytes() != want[1].tobytes()
first = run(r, sync=False)
tpt.set_scene(s2, m2)
tpt.UpdateTest(0.0, 0, W, H, 0)
second = run(r, sync=False)
tpt.set_scene(None, None)
tpt.synchronize()
check(first, want, "the old scene")
check(second, want2, "the new scene")
tpt.UpdateTest(0.0, 0, W, H, 0)
check(run(r), want, "the built-in scene again")
print("accepted: a scene set behind a running call")

# records the statement is not defined for: the run ends, and every other ray is the checker's
bad = np.ascontiguousarray(cam_rays[:200]).copy()
idx = {3: (0, np.nan), 17: (1, np.inf), 40: (4, np.nan), 41: (5, -np.inf), 64: (4, 0.0), 65: (2, 1e38), 130: (6, 3e38)}
for i, (k, v) in idx.items():
    bad[i, k] = v
bad[64, 4:7] = 0  # a zero direction
bad[66, 4:7] = 0
bad[66, 0:3] = (s["cx"][7], s["cy"][7], s["cz"][7])  # ... from inside a sphere
for hs in (0, 1):
    tpt.set_kernel_variant(hs, 3, -1)
    out = run(bad)
    clean = np.ones(200, bool)
    clean[list(idx) + [66]] = False
    w = checker.trace(s, m, np.ascontiguousarray(cam_rays[:200]))
    assert out["rad"][1:-1][clean].tobytes() == w[1][clean].tobytes() and out["hit"][1:-1][clean].tobytes() == w[2][clean].tobytes()
    assert np.isnan(out["rad"][0]).all() and np.isnan(out["rad"][-1]).all()
tpt.set_kernel_variant(0, 3, -1)
print("accepted: non-finite and zero-direction records")

# the context around a call: a synchronous caller's frames (traced ahead of its calls from the third on) with ray calls in between
def frames(with_calls):
    tpt.set_samples_per_pixel(2)
    tile = np.zeros((H * 4, W * 4, 4), np.float32)
    hits0, r0 = tpt.lookahead_hits(), tpt.ray_counter_read()
    for f in range(8):
        tpt.UpdateTest(0.0, f, W * 4, H * 4, FLAG_PROGRESSIVE)
        tpt.draw_device(0.0, f, W * 4, H * 4, ptr(tile), FLAG_PROGRESSIVE)
        tpt.synchronize()
        if with_calls and f in (4, 5):
            before = [a.tobytes() for a in tpt.GetSceneDesc()] + [tpt.lookahead_hits(), tpt.ray_counter_read(), tpt.pipeline_info()]
            check(run(r), want, "between frames")
            assert [a.tobytes() for a in tpt.GetSceneDesc()] + [tpt.lookahead_hits(), tpt.ray_counter_read(), tpt.pipeline_info()] == before
    return tile.tobytes(), tpt.lookahead_hits() - hits0, tpt.ray_counter_read() - r0
a, b = frames(True), frames(False)
assert a == b and a[1] > 0, (a[1:], b[1:])
total, img, _ = oracle_frames(Oracle.get(), W * 4, H * 4, 2, 8, seed_mode=SEED_PER_PIXEL)
assert a[0] == img.tobytes() and a[2] == total
print("accepted: frames traced ahead are kept")
# ... and an open stream batch: frames enqueued without a wait, a ray call in their middle
def stream(with_call):
    tile = np.zeros((H * 4, W * 4, 4), np.float32)
    r0 = tpt.ray_counter_read()
    out = None
    for f in range(12):
        tpt.UpdateTest(0.0, f, W * 4, H * 4, FLAG_PROGRESSIVE)
        tpt.draw_device(0.0, f, W * 4, H * 4, ptr(tile), FLAG_PROGRESSIVE)
        if with_call and f == 6:
            out = run(r, sync=False)
    tpt.synchronize()
    if out:
        check(out, want, "inside a stream of frames")
    return tile.tobytes(), tpt.ray_counter_read() - r0
a, b = stream(True), stream(False)
total, img, _ = oracle_frames(Oracle.get(), W * 4, H * 4, 2, 12, seed_mode=SEED_PER_PIXEL)
assert a == b and a[0] == img.tobytes() and a[1] == total
print("accepted: a stream of frames is kept")
tpt.ShutdownTest()
print("ok")
'''


def run_script(mode, policy):
    from test_host_logic import build
    path = build("libtpt_hostemu_rays.so", [os.path.join(ROOT, "tests", "hostemu_rays.cpp")])
    env = dict(os.environ, TPT_LIB=path, HOSTEMU_POLICY=policy)
    env.pop("TPT_LIB_DIR", None)
    return subprocess.Popen([sys.executable, "-c", SCRIPT, ROOT, mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def finish(p):
    out = p.communicate(timeout=900)[0].decode()
    assert p.returncode == 0 and out.rstrip().endswith("ok"), out[-4000:]
    return out


def test_refusals_through_the_host_runtime():
    out = finish(run_script("refusals", "lazy"))
    assert out.count("refused:") == 1 + 1 + 1 + 4 + 3 + 1 + 1 + 11 + 2, out
    assert "accepted: buffers that touch" in out
    assert out.count("order:") == 7 + 2, out
    assert refusal_messages(out) == {
        "tpt: not initialised (call tptInitialize / InitializeTest first)": 1,
        NAME + ": call tptUpdate first": 1,
        NAME + ": args is required": 1,
        NAME + ": nRays must lie in 1..16777216": 4,
        NAME + ": flags must be 0": 3,
        NAME + ": deviceRays is required": 1,
        NAME + ": deviceRadiance or deviceHits is required": 1,
        NAME + ": an output overlaps deviceRays": 7,
        NAME + ": two outputs overlap": 4,
        NAME + ": too many emissive spheres for the LDS light table (3072 at most)": 1,
        NAME + ": scene too large for LDS staging; use tptSetKernelVariant(.., .., 0)": 1,
    }


@pytest.fixture(scope="module")
def schedules():
    """the three schedules at once, one process each"""
    jobs = {policy: run_script("accepted", policy) for policy in ("eager", "lazy", "random:3")}
    return {policy: finish(p) for policy, p in jobs.items()}


@pytest.mark.parametrize("policy", ["eager", "lazy", "random:3"])
def test_accepted_calls_equal_the_checker(schedules, policy):
    out = schedules[policy]
    assert "accepted: 56 calls equal the checker" in out, out
    for line in ("the spill grows between calls", "the ray counts", "three calls back to back", "a scene set behind a running call", "non-finite and zero-direction records",
                 "frames traced ahead are kept", "a stream of frames is kept"):
        assert "accepted: " + line in out, out


def test_a_build_without_the_launcher_refuses():
    """the host runtime with the emulated kernels alone: tptLaunchTraceRays is a weak symbol nobody defines"""
    script = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
from toypathtracer_amd.scenes import cloud_scene
tpt.InitializeTest()
rays, rad = np.ones((4, 8), np.float32), np.full((4, 4), np.nan, np.float32)
a = tpt.TraceRaysArgs(nRays=4, flags=0, deviceRays=rays.ctypes.data, deviceRadiance=rad.ctypes.data, deviceHits=None, deviceRayCount=None)
# the launcher is looked for last: a scene whose LDS does not fit is still refused as that
s, m = cloud_scene(3000)
tpt.set_scene(s, m)
tpt.set_kernel_variant(2, 1, 1)
tpt.UpdateTest(0.0, 0, 16, 8, 0)
assert lib.tptTraceRaysDevice(C.byref(a)) != 0
m = lib.tptGetLastError().decode()
assert m == "tptTraceRaysDevice: scene too large for LDS staging; use tptSetKernelVariant(.., .., 0)", m
tpt.set_kernel_variant(0, 3, -1)
tpt.set_scene(None, None)
tpt.UpdateTest(0.0, 0, 16, 8, 0)
assert lib.tptTraceRaysDevice(C.byref(a)) != 0
m = lib.tptGetLastError().decode()
assert "tptTraceRaysDevice" in m and "launcher" in m, m
assert m == "tptTraceRaysDevice: this build has no ray launcher", m
tpt.synchronize()
assert np.isnan(rad).all()
tpt.ShutdownTest()
print("ok")
'''
    run_refusals(script)
