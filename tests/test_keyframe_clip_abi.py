"""tptDrawDeviceKeyframeClip without a GPU: the declaration, the binding and the export of the entry point; the binding's argument checks;
the gfx950 code of the keyframe kernels (tptKeyframeKernel: the camera-clip kernel with the caller's centres per frame read from an LDS
table and a launch-uniform mask of the moved spheres) in the shipped library, held to the queue-kernel contract and to the register
ceilings of the camera-clip kernels; tptQueueVariant and tptQueueLdsBytes compiled for the host; and the refusals, driven through the host
runtime compiled against tests/hostemu (a refused call returns before anything is enqueued)."""
import os
import re
import subprocess

import pytest

from isa_lib import code_object, count, exported_symbols, header_params, no_library, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import CAMERA_CLIP, KEYFRAME, QUEUE, family
from oracle_lib import ROOT

NAME = "tptDrawDeviceKeyframeClip"


def test_header_declares_the_entry_point():
    assert header_params(NAME) == ["int firstFrame", "int nFrames", "const float* views", "int nMoved", "const int32_t* movedIds",
                                   "const float* centres", "int screenWidth", "int screenHeight", "float* deviceTile",
                                   "float* deviceMoments", "float* deviceFrameImages", "float* deviceFrameAlbedo",
                                   "float* deviceFrameNormalDepth", "float* deviceFrameMoments", "int64_t* deviceFrameRays",
                                   "int32_t* deviceFrameObjects", "void* outCameras", "unsigned testFlags"]


def test_binding_and_export():
    from toypathtracer_amd import api
    assert NAME in api.C_ABI_SYMBOLS
    assert callable(api.draw_device_keyframe_clip)
    lib = api.load_library()
    assert hasattr(lib, NAME)
    assert len(getattr(lib, NAME).argtypes) == len(header_params(NAME))
    assert re.search(r"\bT %s\b" % NAME, exported_symbols(api.library_path()))


VIEW = [0.0, 2.0, 3.0, 0.0, 0.0, 0.0, 60.0, 0.02, 3.0]
CENTRE = [0.0, 1.0, 0.0]


def np_shape(v):
    import numpy as np
    return np.asarray(v).shape


@pytest.mark.parametrize("args", [
    dict(views=VIEW), dict(views=[VIEW[:8]] * 2), dict(views=[[VIEW, VIEW]]), dict(ids=[[1, 8]]), dict(ids=[1.0, 8.0]), dict(ids=[1]),
    dict(ids=[1, 8, 9]), dict(centres=[CENTRE, CENTRE]), dict(centres=[[CENTRE, CENTRE]]), dict(centres=[[CENTRE] * 2] * 3),
    dict(centres=[[CENTRE[:2]] * 2] * 2), dict(ids=[], centres=[[CENTRE] * 2] * 2), dict(w=0), dict(h=-3), dict(w=8.0), dict(tile=0),
    dict(tile=None), dict(mo=None), dict(mo=0), dict(mo=1.5), dict(images="x"), dict(albedo=-16), dict(nd=2.0), dict(fm=True),
    dict(rays="x"), dict(objects=-4), dict(objects=1.0),
], ids=lambda a: ",".join("%s=%r" % (k, v if k not in ("views", "centres") else np_shape(v)) for k, v in a.items()))
def test_binding_checks_arguments_before_the_library(monkeypatch, args):
    """views (N, 9), moved_ids (K,) of integers, centres (N, K, 3); the sizes and pointers as draw_device_camera_clip checks them"""
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(views=[VIEW, VIEW], ids=[1, 8], centres=[[CENTRE] * 2] * 2, w=16, h=8, tile=4096, mo=8192, images=None, albedo=None, nd=None,
             fm=None, rays=None, objects=None)
    a.update(args)
    with pytest.raises(ValueError):
        api.draw_device_keyframe_clip(a["views"], a["ids"], a["centres"], 0, a["w"], a["h"], a["tile"], a["mo"], 2, images_ptr=a["images"],
                                      albedo_ptr=a["albedo"], normal_depth_ptr=a["nd"], frame_moments_ptr=a["fm"], rays_ptr=a["rays"],
                                      objects_ptr=a["objects"])


# ---------------------------------------------------------------- the shipped gfx950 code
@pytest.mark.parametrize("lds", [1, 0], ids=["lds-scene", "flat-global"])
def test_keyframe_kernels_keep_the_queue_kernel_contract(code_object, lds):  # noqa: F811
    bodies, meta = code_object
    name = KEYFRAME % lds
    assert name in meta and name in bodies, "the keyframe kernel is missing from the shipped code object"
    body, m = bodies[name], meta[name]
    assert count(body, r"flat_") == 0, "a FLAT instruction: an LDS pointer lost its address space"
    assert count(body, r"buffer_(load|store|atomic)") == 0
    assert m["agpr_count"] == 0
    assert m["max_flat_workgroup_size"] == 512 and m["wavefront_size"] == 64
    # the matrix-core filter of its single-frame twin (8 MFMA for the <= 64-sphere table), none without the scene in LDS
    twin = QUEUE % (lds, 0)
    assert count(body, r"v_mfma") == count(bodies[twin], r"v_mfma") == (8 if lds else 0)
    # the LDS of its single-frame twin: both tables replace path records, the sums live in global memory
    assert m["group_segment_fixed_size"] == meta[twin]["group_segment_fixed_size"] == meta[CAMERA_CLIP % lds]["group_segment_fixed_size"]
    # the ceiling the camera-clip kernels are held to (128 VGPRs / 6 spilled / 28 B of scratch; with the scene in LDS 120 VGPRs, so that
    # the resolve kernel's waves start beside it)
    assert m["vgpr_count"] <= (120 if lds else 128), m
    assert m["vgpr_spill_count"] <= 6 and m["private_segment_fixed_size"] <= 28, m
    # every plane store of the camera-clip kernel
    assert count(body, r"global_store_dwordx4") >= count(bodies[CAMERA_CLIP % lds], r"global_store_dwordx4")


def test_exactly_one_new_kernel_pair(code_object):  # noqa: F811
    _, meta = code_object
    assert sorted(n for n in meta if "Keyframe" in n) == sorted(family(KEYFRAME))


# ---------------------------------------------------------------- the variant decision and the LDS of a launch, on the host
VARIANT_PROGRAM = r'''
#include <cstdio>
#include <initializer_list>
#include "tpt_queue_layout.h"
using namespace tpt;
int main()
{
    static CameraPOD cams[32];
    static f4 keyed[32 * TPT_Q_KEYS_MAX], centres[64], sums[3], plane[1];
    static int32_t counts[1];
    KernelArgs a{};
    a.scene.nPairs = 23; a.scene.nSpheres = 46; a.scene.nLights = 2; a.scene.mxR1 = 0; // (the built-in scene)
    a.batchFrames = 1;
    const size_t single = tptQueueLdsBytes(a, true), singleFlat = tptQueueLdsBytes(a, false);
    printf("single %d\n", (int)(tptQueueVariant(a) == QV_FRAME));
    a.batchFrames = 32;
    a.viewCams = cams; a.keyCentres = keyed; a.keyMask = 0xC100000000000001ull; a.keyCount = 4; a.aovSums = sums; a.momentsOut = plane;
    printf("keys %d %d\n", (int)tptQueueVariant(a), (int)QV_KEYFRAME_CLIP);
    printf("lds %zu %zu %zu %zu\n", tptQueueLdsBytes(a, true), single, tptQueueLdsBytes(a, false), singleFlat);
    printf("two_per_cu %d\n", (int)(160 * 1024 / (tptQueueLdsBytes(a, true) + 256)));
    printf("table %d %d %d\n", (int)TPT_Q_KEY_TABLE_BYTES, (int)TPT_Q_KEY_PATHS, (int)TPT_Q_VIEW_PATHS);
    for (int n : {1, 17}) { a.batchFrames = n; printf("frames %d %d\n", n, (int)tptQueueVariant(a)); }
    for (int n : {0, 33}) { a.batchFrames = n; printf("invalid frames %d %d\n", n, (int)(tptQueueVariant(a) == QV_INVALID)); }
    a.batchFrames = 32;
    a.keyCount = 0; a.keyMask = 0; printf("nothing-moved %d\n", (int)(tptQueueVariant(a) == QV_KEYFRAME_CLIP));
    a.keyCount = 9; printf("invalid nine %d\n", (int)(tptQueueVariant(a) == QV_INVALID)); a.keyCount = 4;
    a.viewCams = nullptr; printf("invalid no-cameras %d\n", (int)(tptQueueVariant(a) == QV_INVALID)); a.viewCams = cams;
    a.momentsOut = nullptr; printf("invalid no-moments %d\n", (int)(tptQueueVariant(a) == QV_INVALID)); a.momentsOut = plane;
    a.aovSums = nullptr; printf("invalid no-sums %d\n", (int)(tptQueueVariant(a) == QV_INVALID));
    a.momentsOut = nullptr; printf("invalid no-planes %d\n", (int)(tptQueueVariant(a) == QV_INVALID));
    a.aovSums = sums; a.momentsOut = plane;
    a.moveCentres = centres; printf("invalid both-tables %d\n", (int)(tptQueueVariant(a) == QV_INVALID)); a.moveCentres = nullptr;
    a.sampleCounts = counts; printf("invalid counts %d\n", (int)(tptQueueVariant(a) == QV_INVALID)); a.sampleCounts = nullptr;
    a.scene.nGroups = 4; printf("invalid grouped %d\n", (int)(tptQueueVariant(a) == QV_INVALID)); a.scene.nGroups = 0;
    a.keyCentres = nullptr; a.moveCentres = centres; printf("camera-clip %d\n", (int)(tptQueueVariant(a) == QV_CAMERA_CLIP));
    a.viewCams = nullptr; printf("clip %d\n", (int)(tptQueueVariant(a) == QV_CLIP));
    printf("valid %d\n", (int)(QV_KEYFRAME_CLIP < QV_INVALID));
    return 0;
}
'''


def test_variant_and_lds_on_the_host(tmp_path):
    src, exe = str(tmp_path / "variant.cpp"), str(tmp_path / "variant")
    open(src, "w").write(VARIANT_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-include", "hip/hip_runtime.h",
                           "-I", os.path.join(ROOT, "tests", "hostemu"), "-I", os.path.join(ROOT, "toypathtracer_amd", "csrc"), src, "-o", exe])
    out = dict(ln.rsplit(" ", 1) if not ln.startswith(("keys", "lds", "table")) else (ln.split()[0], ln.split()[1:])
               for ln in subprocess.check_output([exe]).decode().splitlines())
    assert out["single"] == "1"
    assert out["keys"][0] == out["keys"][1], "the key table with the cameras and the planes selects the keyframe variant"
    assert out["frames 1"] == out["frames 17"] == out["keys"][0]
    assert out["nothing-moved"] == "1", "a clip in which nothing moves rides the same kernel"
    for case in ("frames 0", "frames 33", "nine", "no-cameras", "no-moments", "no-sums", "no-planes", "both-tables", "counts", "grouped"):
        assert out["invalid " + case] == "1", case
    assert out["camera-clip"] == "1" and out["clip"] == "1", "the existing decisions stand"
    assert out["valid"] == "1"
    lds, single, flat, single_flat = (int(v) for v in out["lds"])
    assert lds == single and flat == single_flat, "the LDS of a launch is its single-frame twin's"
    assert out["two_per_cu"] == "2"
    assert out["table"] == ["4096", "64", "44"], "32 x 8 x 16 B in the place of exactly 64 path records, on top of the cameras' 44"


# ---------------------------------------------------------------- which centre a sphere reads, on the host
SLOT_PROGRAM = r'''
#include <cstdio>
#include <cstdint>
#include "tpt_queue_layout.h"
using namespace tpt;
int main()
{
    // every set of up to TPT_Q_KEYS_MAX ids drawn by a small generator, ids 0 and 63 among them: a moved sphere reads the centre at its
    // rank among the moved ids (.w kept), every other sphere -- those of index 64 and above too -- keeps its record
    uint32_t rng = 12345u;
    int bad = 0, sets = 0;
    for (int trial = 0; trial < 2000; ++trial) {
        uint64_t mask = 0;
        const int want = trial % (TPT_Q_KEYS_MAX + 1);
        int have = 0;
        while (have < want) {
            rng = rng * 1664525u + 1013904223u;
            int id = (int)((rng >> 8) % 64u);
            if (trial % 7 == 0 && have == 0) id = 0;
            if (trial % 5 == 0 && have == 1 && !(mask & 1ull)) id = 63;
            if (mask & (1ull << (63 - id))) continue;
            mask |= 1ull << (63 - id);
            ++have;
        }
        f4 table[TPT_Q_KEYS_MAX];
        for (int k = 0; k < TPT_Q_KEYS_MAX; ++k) table[k] = f4{100.0f + k, 200.0f + k, 300.0f + k, -1.0f};
        int rank = 0;
        for (int id = 0; id < 200; ++id) {
            const f4 s = {(float)id, 0.5f, -2.0f, 7.0f};
            const f4 got = keyedSphere(s, id, table, mask);
            const bool moved = id < 64 && (mask & (1ull << (63 - id)));
            const f4 exp = moved ? f4{100.0f + rank, 200.0f + rank, 300.0f + rank, 7.0f} : s;
            if (got.x != exp.x || got.y != exp.y || got.z != exp.z || got.w != exp.w) ++bad;
            if (moved) ++rank;
        }
        if (rank != want) ++bad;
        ++sets;
    }
    printf("sets %d bad %d\n", sets, bad);
    return 0;
}
'''


def test_a_moved_sphere_reads_the_centre_at_its_rank(tmp_path):
    src, exe = str(tmp_path / "slot.cpp"), str(tmp_path / "slot")
    open(src, "w").write(SLOT_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-include", "hip/hip_runtime.h",
                           "-I", os.path.join(ROOT, "tests", "hostemu"), "-I", os.path.join(ROOT, "toypathtracer_amd", "csrc"), src, "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["sets", "2000", "bad", "0"]


# ---------------------------------------------------------------- the keyed intersection against the exact loop, on the host
HIT_PROGRAM = r'''
#include <cstdio>
#include <cstdint>
#include "tpt_scene.h"
using namespace tpt;
enum { kKeys = 8 }; // (TPT_Q_KEYS_MAX: the centres of a frame in the table)
static uint32_t rng = 99u;
static float uni(float lo, float hi) { rng = rng * 1664525u + 1013904223u; return lo + (hi - lo) * (float)(rng >> 8) * (1.0f / 16777216.0f); }
int main()
{
    // the default scene (46 spheres, one chunk) and a flat one of 200 (four chunks: the mask touches the first only).  The staged scene
    // is the LAST frame's, as a launch stages it; frame j's rays are intersected with the staged filter, the mask and frame j's table,
    // and must find what the exact loop over S_j finds: the same sphere at the same t.
    long long rays = 0, bad = 0, hits = 0, onMoved = 0;
    for (int big = 0; big < 2; ++big) {
        std::vector<SpherePOD> base;
        std::vector<MaterialPOD> mats;
        defaultScene(base, mats);
        if (big)
            for (int i = 46; i < 200; ++i) {
                SpherePOD s = base[9 + i % 30];
                s.cx = uni(-8.0f, 8.0f); s.cz = uni(-8.0f, 8.0f);
                base.push_back(s);
                mats.push_back(mats[9 + i % 30]);
            }
        const int ids[kKeys] = {big ? 63 : 45, 0, 8, 1, 3, 7, 2, big ? 62 : 4};
        const int frames = 5;
        uint64_t mask = 0;
        for (int k = 0; k < kKeys; ++k) mask |= 1ull << (63 - ids[k]);
        std::vector<std::vector<SpherePOD>> S(frames, base);
        f4 table[frames][kKeys];
        for (int j = 0; j < frames; ++j)
            for (int k = 0; k < kKeys; ++k) {
                SpherePOD& s = S[j][ids[k]];
                s.cx += uni(-0.3f, 0.3f); s.cy += uni(-0.3f, 0.3f); s.cz += uni(-0.3f, 0.3f);
                int slot = 0;
                for (int m = 0; m < kKeys; ++m) slot += ids[m] < ids[k];
                table[j][slot] = f4{s.cx, s.cy, s.cz, 0.0f};
            }
        PackedScene staged, own;
        packScene(S[frames - 1], mats, staged);
        const SceneView sv = viewOf(staged);
        for (int j = 0; j < frames; ++j) {
            packScene(S[j], mats, own);
            const SceneView exact = viewOf(own);
            for (int r = 0; r < 20000; ++r) {
                const f3 o = mk3(uni(-4.0f, 4.0f), uni(0.1f, 3.0f), uni(-4.0f, 4.0f));
                const f3 d = normalize(mk3(uni(-1.0f, 1.0f), uni(-1.0f, 0.4f), uni(-1.0f, 1.0f)));
                float t0 = 0, t1 = 0, t2 = 0;
                const int want = hitSpheresSimple(exact, o, d, TPT_MIN_T, TPT_MAX_T, t0);
                const int got = hitSpheresTwoPhase<true, true>(sv, o, d, TPT_MIN_T, TPT_MAX_T, t1, table[j], mask);
                bad += got != want || (want >= 0 && t1 != t0);
                if (!big) { // (a scene of one chunk: phase 2 over a mask, as behind the matrix-core filter -- here the packed filter's mask)
                    const v2f ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z};
                    const float kx = d.x * TPT_P1_K, ky = d.y * TPT_P1_K, kz = d.z * TPT_P1_K;
                    const v2f dx = {kx, kx}, dy = {ky, ky}, dz = {kz, kz};
                    const uint64_t cand = phase1Chunk(pairPtr(sv.pairs), sv.nPairs, ox, oy, oz, dx, dy, dz);
                    const int got2 = hitSpheresCandidates<true, true>(sv, cand, o, d, TPT_MIN_T, TPT_MAX_T, t2, table[j], mask);
                    bad += got2 != want || (want >= 0 && t2 != t0);
                }
                ++rays;
                hits += want >= 0;
                for (int k = 0; k < kKeys; ++k) onMoved += want == ids[k] && want != 0;
                // the hit normal on a moved sphere comes from the frame's centre
                if (want >= 0) {
                    const f3 p = o + d * t0;
                    const f3 n0 = qNormal(exact, want, p), n1 = qNormal<true, true>(sv, want, p, table[j], mask);
                    bad += n0.x != n1.x || n0.y != n1.y || n0.z != n1.z;
                }
            }
        }
    }
    printf("rays %lld hits %lld on-moved %lld bad %lld\n", rays, hits, onMoved, bad);
    return 0;
}
'''


def test_keyed_intersection_equals_the_exact_loop_over_each_frames_spheres(tmp_path):
    """tpt_trace.h compiled for the host: the staged filter of a launch's last frame, the mask and a frame's table find, for 200 000
    rays over five frames of two scenes, the sphere and the distance the reference's loop finds over that frame's own spheres"""
    src, exe = str(tmp_path / "hit.cpp"), str(tmp_path / "hit")
    open(src, "w").write(HIT_PROGRAM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "toypathtracer_amd", "csrc"),
                           src, "-o", exe])
    out = subprocess.check_output([exe]).decode().split()
    assert out[0] == "rays" and int(out[1]) == 200000 and out[-2:] == ["bad", "0"], out
    assert int(out[3]) > 100000 and int(out[5]) > 2000, out  # (most rays hit something, thousands of them a moved sphere other than the ground)


# ---------------------------------------------------------------- refusals, through the host runtime
REFUSALS = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
w, h, n = 16, 8, 3
plane = w * h * 16
tile = np.full((h, w, 4), 7.25, np.float32)
mo = np.full((h, w, 4), 0.5, np.float32)
images = np.full((n, h, w, 4), -1.5, np.float32)
alb = np.full((n, h, w, 4), 0.25, np.float32)
nd = np.full((n, h, w, 4), 3.0, np.float32)
fmo = np.full((n, h, w, 4), -0.75, np.float32)
rays = np.full(n, -5, np.int64)
objs = np.full((n, h, w), -9, np.int32)
big = np.zeros((2 * n, h, w, 4), np.float32)
cams = np.full(12 * 88, 0xA5, np.uint8)
views = np.float32([[3.0 * np.sin(0.1 * j), 2.0, 3.0 * np.cos(0.1 * j), 0.0, 0.0, 0.0, 50.0, 0.05, 2.5] for j in range(12)])
ids = np.int32([0, 45, 7, 1])
centres = np.float32(np.arange(12 * 4 * 3).reshape(12, 4, 3) % 5)
ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
F = "tptDrawDeviceKeyframeClip"
def call(ww=w, hh=h, nn=n, v=views, k=4, i=ids, c=centres, tl=tile, m=mo, im=images, a=alb, d=nd, fm=fmo, r=rays, o=objs, cm=cams, fl=2):
    return lib.tptDrawDeviceKeyframeClip(0, nn, ptr(v), k, ptr(i), ptr(c), ww, hh, ptr(tl), ptr(m), ptr(im), ptr(a), ptr(d), ptr(fm), ptr(r),
                                         ptr(o), ptr(cm), fl)
def scene_desc():
    s, cam = np.zeros(tpt.GetObjectCount()[0] * 5, np.float32), np.zeros(22, np.float32)
    lib.tptGetSceneDesc(s.ctypes.data, None, cam.ctypes.data, None, None)
    return s.tobytes() + cam.tobytes()
state = None
def refused(what, expect=F, **kw):
    rc = call(**kw)
    msg = lib.tptGetLastError().decode()
    assert rc != 0 and expect in msg, (what, rc, msg)
    assert (cams == 0xA5).all(), (what, "outCameras written")
    assert state is None or scene_desc() == state, (what, "the camera or the spheres changed (tptGetSceneDesc)")
    print("refused:", what, "--", msg)
def reset():
    tpt.set_seed_mode(1); tpt.set_fold_mode(0); tpt.set_kernel_variant(0, 3, -1); tpt.set_row_shard(0, 1, 0); tpt.set_samples_per_pixel(4)
def update(ww, hh):
    global state
    tpt.UpdateTest(0.0, 0, ww, hh, 2)
    state = scene_desc()
refused("no context", "not initialised")
tpt.InitializeTest()
refused("before any tptUpdate")
update(w, h)
# ---- what tptDrawDeviceCameraClip refuses that still applies
refused("0 frames", nn=0)
refused("-1 frames", nn=-1)
refused("views NULL", v=None)
refused("tile NULL", tl=None)
refused("moments NULL", m=None)
refused("no tptUpdate at this size", hh=h + 1)
refused("width 0", ww=0)
refused("height 0", hh=0)
refused("height -1", hh=-1)
update(8200, 8)
refused("wider than 8192", ww=8200, hh=8)
update(8192, 8192)
refused("12 GiB of colour", ww=8192, hh=8192, nn=12)
refused("6 GiB of colour and moments (the colour alone would pass)", ww=8192, hh=8192, nn=3)
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
# (65535 spheres: one more than the path-queue kernel's ids hold; the moved ids themselves are good ones)
many = np.zeros(65535, tpt.SPHERE_DT)
many["cx"], many["cz"] = np.arange(65535) % 256 - 128.0, np.arange(65535) // 256 - 128.0
many["radius"], many["invRadius"] = 0.25, 4.0
manyMats = np.zeros(65535, tpt.MATERIAL_DT)
manyMats["albedo"] = 0.5
tpt.set_scene(many, manyMats)
update(w, h)
assert tpt.GetObjectCount()[0] == 65535
refused("65535 spheres", expect=F + ": at most 65534 spheres")
refused("65535 spheres, nothing moved", expect=F + ": at most 65534 spheres", k=0, i=None, c=None)
tpt.set_scene(None)
update(w, h)
assert tpt.GetObjectCount()[0] == 46
# ---- its own
refused("nMoved -1", k=-1)
refused("nMoved 47 of 46 spheres", k=47, i=np.arange(47, dtype=np.int32), c=np.zeros((12, 47, 3), np.float32))
refused("movedIds NULL", i=None)
refused("centres NULL", c=None)
refused("an id of -1", i=np.int32([0, 45, -1, 1]))
refused("an id of 46", i=np.int32([0, 46, 7, 1]))
refused("a repeated id", i=np.int32([0, 45, 7, 45]))
bad = centres.copy(); bad[2, 3, 1] = np.nan
refused("a NaN centre", c=bad)
bad[2, 3, 1] = -np.inf
refused("an infinite centre", c=bad)
refused("kFlagAnimate", fl=1)
refused("kFlagAnimate | kFlagProgressive", fl=3)
refused("flag bit 4", fl=6)
nanView = views.copy(); nanView[1, 0] = np.nan
refused("object planes with a view whose camera is not finite", v=nanView)
# ---- any two of the eight buffers overlapping, each at its full extent
refused("moments is the tile", m=tile)
refused("images start at the tile", im=tile)
refused("albedo is the normal / depth", a=nd)
refused("frame moments are the moments", fm=mo)
refused("frame moments are the images", fm=images)
refused("moments inside the albedo's last plane", m=alb.ctypes.data + 2 * plane + 16)
refused("the tile is the last pixel of the frame moments", tl=fmo.ctypes.data + 3 * plane - 16)
refused("normal / depth starts in the images' last plane", im=big, d=big.ctypes.data + 3 * plane - 16)
refused("the rays lie in the images", r=images.ctypes.data + plane)
refused("the albedo starts in the rays", a=rays.ctypes.data + 8 * n - 8)
refused("the object planes are the tile", o=tile)
refused("the object planes end in the images", o=images.ctypes.data - 3 * w * h * 4 + 4)
refused("the rays lie in the object planes", r=objs.ctypes.data + 2 * w * h * 4)
refused("the moments start in the object planes' last plane", m=objs.ctypes.data + 3 * w * h * 4 - 16)
tpt.synchronize()
assert (tile == 7.25).all() and (mo == 0.5).all() and (images == -1.5).all() and (alb == 0.25).all() and (nd == 3.0).all(), "a refused call wrote"
assert (fmo == -0.75).all() and list(rays) == [-5] * n and (big == 0.0).all() and (cams == 0xA5).all() and (objs == -9).all(), "a refused call wrote"
# ---- accepted: buffers that touch without sharing a byte; nothing moved; eight moved spheres given out of order.  The emulated
#      object-plane launcher keeps what the host handed it: a launch per frame, each with the frame's centres of spheres 1 and 8
so = C.CDLL(tpt.library_path())
so.hostemuObjectPlaneConsts.restype = C.POINTER(C.c_float * 18)
so.hostemuObjectPlaneConsts.argtypes = [C.c_int]
so.hostemuObjectPlaneOut.restype = C.c_void_p
assert so.hostemuObjectPlaneLaunches() == 0, "a refused call reached the object-plane launcher"
assert call(im=big, d=big.ctypes.data + 3 * plane, k=0, i=None, c=None) == 0, lib.tptGetLastError().decode()
tpt.synchronize()
assert so.hostemuObjectPlaneLaunches() == n and (cams[:n * 88] != 0xA5).any() and (cams[n * 88:] == 0xA5).all()
after = scene_desc()
assert after[:46 * 20] == state[:46 * 20], "nothing moved, and the spheres changed"
assert np.frombuffer(after[46 * 20:], np.float32).tobytes() == cams[(n - 1) * 88:n * 88].tobytes(), "the camera is not the last view's"
print("accepted: adjacent buffers, nothing moved")
ids8 = np.int32([45, 8, 0, 30, 1, 17, 2, 9])
c8 = np.float32(np.random.default_rng(5).uniform(-2.0, 2.0, (n, 8, 3)))
before = np.frombuffer(scene_desc()[:46 * 20], np.float32).reshape(46, 5).copy()
first = so.hostemuObjectPlaneLaunches()
assert call(k=8, i=ids8, c=c8) == 0, lib.tptGetLastError().decode()
tpt.synchronize()
assert so.hostemuObjectPlaneLaunches() == first + n
for j in range(n):
    k = np.array(so.hostemuObjectPlaneConsts(first + j).contents, np.float32)
    assert k[:12].tobytes() == cams[j * 88:j * 88 + 48].tobytes(), "frame %d's object plane is not traced through its camera" % j
    assert k[12:15].tobytes() == c8[j, 4].tobytes() and k[15:18].tobytes() == c8[j, 1].tobytes(), "frame %d: the centres of spheres 1 and 8" % j
    assert so.hostemuObjectPlaneSpheres(first + j) == 46 and so.hostemuObjectPlaneOut(first + j) == objs.ctypes.data + 4 * w * h * j
want = before.copy()
want[ids8, :3] = c8[n - 1]
got = np.frombuffer(scene_desc()[:46 * 20], np.float32).reshape(46, 5)
assert got.tobytes() == want.tobytes(), "the context's spheres are not S_{n-1}"
print("accepted: eight moved spheres")
# (nine moved spheres go frame by frame: a launch and a sphere array per frame, the arrays' two halves taken in turn)
ids9 = np.int32([45, 8, 0, 30, 1, 17, 2, 9, 5])
c9 = np.float32(np.random.default_rng(6).uniform(-2.0, 2.0, (n, 9, 3)))
first = so.hostemuObjectPlaneLaunches()
assert call(k=9, i=ids9, c=c9) == 0, lib.tptGetLastError().decode()
tpt.synchronize()
assert so.hostemuObjectPlaneLaunches() == first + n
for j in range(n):
    k = np.array(so.hostemuObjectPlaneConsts(first + j).contents, np.float32)
    assert k[:12].tobytes() == cams[j * 88:j * 88 + 48].tobytes() and so.hostemuObjectPlaneSpheres(first + j) == 46
    assert k[12:15].tobytes() == c9[j, 4].tobytes() and k[15:18].tobytes() == c9[j, 1].tobytes(), "frame %d: the centres of spheres 1 and 8" % j
want[ids9, :3] = c9[n - 1]
assert np.frombuffer(scene_desc()[:46 * 20], np.float32).tobytes() == want.tobytes(), "the context's spheres are not S_{n-1}"
print("accepted: nine moved spheres, frame by frame")
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_through_the_host_runtime():
    out = run_refusals(REFUSALS, "libtpt_hostemu_objects.so", ["hostemu_objects.cpp"])
    assert out.count("refused:") == 2 + 12 + 3 + 5 + 2 + 12 + 1 + 14, out
    assert out.count("accepted:") == 3, out
