"""TEST INFRASTRUCTURE: frames at the LIMITS OF THE PACKED FIELDS of the path-queue kernel, for tests/test_seams.py (the oracle, the host's
routing on the emulated runtime and the arithmetic of the table below, on the CPU) and tests/test_gpu_seams.py (the trace kernels on the GPU).
The path-queue kernel keeps integers in float-typed LDS words (u2f / f2u); the host routes a launch to the lane-refill kernel, or refuses it,
by what those fields hold.  Nothing under toypathtracer_amd/ imports this module.

  word                      packing                                         limit                      where the host holds it
  ------------------------  ----------------------------------------------  -------------------------  ---------------------------------------
  path record               sample & 0x7ff | depth << 11 | doMatE << 15     spp <= 2047                tpt_host_pipeline.cpp pathQueueContext
  (st[1 * kPaths + p].w)    | recId << 16  (recId -1 is 0xffff)             nSpheres <= 65534          tpt_host_pipeline.cpp chooseKernel
                            (tpt_kernels.hip, "const uint32_t w = ...")     (past either: tptDrawDevice takes the lane-refill kernel; the
                                                                            planes, clip and batch entry points refuse: checkPathQueueDraw
                                                                            "at most 2047 samples per pixel", "at most 65534 spheres")
  pixel of a single frame   px | py << 16                                   width, height <= 65535     tpt_host_pipeline.cpp chooseKernel
  (colSum[p].w)             (tpt_kernels.hip, "const uint32_t where = ..")  (past it: the lane-refill kernel, without a word)
  pixel of a batched launch px | py << 13 | frame << 26                     8192 x 8192, 32 frames     tpt_host_pipeline.cpp enqueueTrace
                            (the same line, and the pools kernel's own)     (tptDrawDeviceBatch refuses 8193; kMaxBatch frames a launch)
  seed of a batch's frame   pixelSeed(.., fc.frame + laneFrame)             uint32 arithmetic          tpt_kernels.hip
  blend factor              lerpFac = float(frame) / float(frame + 1)       frame <= 2^31 - 2          tpt_scene.h makeFrameConsts

In-range values of these words that are NaN bit patterns (exponent bits all ones, mantissa not zero; the ones whose bit 22 is clear are
signalling) -- a canonicalising instruction, a multiply by one or a maximum on such a word would change a row number or a hit id there
and nowhere else:

  single-frame pixel word   rows 32640..32767 and 65408..65535 (py bits 7..14 make the exponent; row 32640, column 0 is +infinity's bits)
  batched pixel word        rows 7168..8191 of slot 31, and only those (frame bits 26..30 and py bits 10..12 make the exponent)
  path record               sphere ids 32640..32767 (and 65408..65535, of which 65535 is "no hit" and ids up to 65533 exist here)

2^31 - 1 is not a frame number of this catalogue: `frame + 1` overflows int in the reference's own lerp expression (Test.cpp:272), which
the oracle restates, so there is nothing to hold the device to.  The per-workgroup ray counter's move at 2^31 rays is not rendered either.

CASES maps a name (the test id) to its builder; build(name) returns (spheres, mats, camera, w, h, spp, first_frame, frames): the arrays
in oracle_lib's record layouts, `camera` None for the default camera or the keyword arguments of toypathtracer_amd.api.set_camera.
ENTRY[name] says through which call the frames are drawn ("draw", "batch", "batch_moments", "camera_clip"), LAUNCHES[name] the frames of
each launch of a batched case, FLAGS[name] the test flags: kFlagProgressive, except for the "_alone" twins of the frames from 2^31 - 4
on -- lerpFac is exactly 1 from frame 2^25 on (and at 2^24), so a progressive frame leaves the tile what it was and only its ray count
shows the seeds; drawn without the flag (lerpFac = 0) the tile is the frame alone."""
import numpy as np

from oracle_lib import FLAG_PROGRESSIVE, MATERIAL_DT, SPHERE_DT, Oracle
from scene_kinds_lib import DEFAULT_CAMERA, DIELECTRIC, LAMBERT, METAL, oracle_camera  # noqa: F401  (oracle_camera: for the test files)

f32 = np.float32

MAX_SPP = 2047            # the record's 11 bits of sample index
MAX_SPHERES = 65534       # 16 bits of sphere id, 0xffff taken by "no hit"
MAX_EXTENT = 65535        # px | py << 16
MAX_BATCH_EXTENT = 8192   # 13 + 13 bits
MAX_BATCH = 32            # frames a launch (the 6-bit field holds more: the host's kMaxBatch)


# ---------------------------------------------------------------- the three packings, restated
def pack_pixel(px, py):
    return (np.asarray(px, np.uint32) | (np.asarray(py, np.uint32) << np.uint32(16))).astype(np.uint32)


def unpack_pixel(w):
    w = np.asarray(w, np.uint32)
    return w & np.uint32(0xffff), w >> np.uint32(16)


def pack_batch_pixel(px, py, frame):
    px, py, frame = (np.asarray(v, np.uint32) for v in (px, py, frame))
    return (px | (py << np.uint32(13)) | (frame << np.uint32(26))).astype(np.uint32)


def unpack_batch_pixel(w):
    w = np.asarray(w, np.uint32)
    return w & np.uint32(0x1fff), (w >> np.uint32(13)) & np.uint32(0x1fff), w >> np.uint32(26)


def pack_record(sample, depth, do_mat_e, rec_id):
    """rec_id -1 (no hit) is stored as 0xffff"""
    r = np.asarray(rec_id, np.int64).astype(np.uint32) & np.uint32(0xffff)
    return ((np.asarray(sample, np.uint32) & np.uint32(0x7ff)) | ((np.asarray(depth, np.uint32) & np.uint32(15)) << np.uint32(11))
            | (np.asarray(do_mat_e, np.uint32) << np.uint32(15)) | (r << np.uint32(16))).astype(np.uint32)


def unpack_record(w):
    w = np.asarray(w, np.uint32)
    rec = (w >> np.uint32(16)).astype(np.int64)
    return w & np.uint32(0x7ff), (w >> np.uint32(11)) & np.uint32(15), (w >> np.uint32(15)) & np.uint32(1), np.where(rec == 0xffff, -1, rec)


def is_nan_pattern(w):
    w = np.asarray(w, np.uint32)
    return ((w & np.uint32(0x7f800000)) == np.uint32(0x7f800000)) & ((w & np.uint32(0x007fffff)) != 0)


def is_signalling(w):
    return is_nan_pattern(w) & ((np.asarray(w, np.uint32) & np.uint32(0x00400000)) == 0)


# the ranges the docstring names: values of the field whose words are NaN patterns for at least one value of the fields below them
NAN_ROWS_SINGLE = (range(32640, 32768), range(65408, 65536))
NAN_ROWS_BATCH_SLOT_31 = range(7168, 8192)
NAN_SPHERE_IDS = (range(32640, 32768), range(65408, 65536))


# ---------------------------------------------------------------- scenes
def _default():
    s, m = Oracle.get().default_scene()
    return s, m


TALL_CAMERA = dict(DEFAULT_CAMERA, vfov=30.0)  # (the default lens of 60 degrees leaves the top rows of a tall frame to the sky)

# where the built-in scene's spheres stand in the many-sphere scenes: index -> sphere of the built-in scene.  0 the ground, 7 the glass
# sphere, 3 .. 6 the metal ones, 8 and 45 the lights, 14 a Lambert sphere of the rows behind.
PLANTED = {0: 0, 1: 1, 32639: 2, 32640: 7, 32704: 3, 32767: 5, 32768: 4, 65407: 6, 65408: 8, 65533: 45}
PLANTED_LAST = {65534: 14}  # (the 65535-sphere scene's own)


def planted(n):
    return {**PLANTED, **PLANTED_LAST} if n > MAX_SPHERES else dict(PLANTED)


def many_spheres(n):
    """n spheres: the built-in scene's at planted(n), every other index a small sphere of a 256-wide lattice behind them (z <= -9:
    beside and behind what the camera sees of the planted ones), jittered like toypathtracer_amd.scenes.stress_scene's and of radii
    0.2 .. 0.45, so that the planted r = 0.5 stays below three median radii and buildGroups groups them with the rest"""
    def build():
        s0, m0 = _default()
        rng = np.random.default_rng(n)
        s, m = np.zeros(n, SPHERE_DT), np.zeros(n, MATERIAL_DT)
        k = np.arange(n)
        u = rng.random((n, 8), dtype=np.float32)
        r = f32(0.2) + f32(0.25) * u[:, 0]
        s["cx"] = (k % 256 - 128).astype(np.float32) + f32(0.6) * u[:, 1]
        s["cz"] = (-9 - k // 256).astype(np.float32) + f32(0.6) * u[:, 2]
        s["cy"] = r - f32(0.5)
        s["radius"] = r
        m["type"] = np.where(u[:, 3] < 0.6, LAMBERT, np.where(u[:, 3] < 0.85, METAL, DIELECTRIC)).astype(np.int32)
        m["albedo"] = f32(0.1) + f32(0.8) * u[:, 4:7]
        m["roughness"] = np.where(m["type"] == METAL, f32(0.3) * u[:, 7], f32(0)).astype(np.float32)
        m["ri"] = np.where(m["type"] == DIELECTRIC, f32(1.5), f32(0)).astype(np.float32)
        for at, i in planted(n).items():
            s[at], m[at] = s0[i], m0[i]
        s["invRadius"] = f32(1.0) / s["radius"]
        return s, m
    return build


_scenes = {}


def scene(key):
    """"default" or ("many", n): built once, read-only"""
    if key not in _scenes:
        s, m = _default() if key == "default" else many_spheres(key[1])()
        s.setflags(write=False)
        m.setflags(write=False)
        _scenes[key] = (s, m)
    return _scenes[key]


def previous_tile(w, h, seed=7):
    """a finite, non-zero tile for the frames that are blended into something: lerpFac shows in every byte"""
    return (np.random.default_rng(seed).random((h, w, 4), dtype=np.float32) * f32(2) + f32(0.25)).astype(np.float32)


# ---------------------------------------------------------------- the catalogue
CASES, ENTRY, LAUNCHES, FAMILY_OF, FLAGS = {}, {}, {}, {}, {}


def _case(family, name, scene_key, camera, w, h, spp, first_frame=0, frames=1, entry="draw", launches=None, flags=FLAG_PROGRESSIVE):
    assert name not in CASES, name
    CASES[name] = (scene_key, camera, w, h, spp, first_frame, frames)
    ENTRY[name], FAMILY_OF[name], FLAGS[name] = entry, family, flags
    if launches is not None:
        assert sum(launches) == frames and max(launches) <= MAX_BATCH
        LAUNCHES[name] = tuple(launches)


for _spp in (17, 1024, 2046, 2047, 2048, 2049):
    _case("samples", "spp_%d" % _spp, "default", None, 8, 8, _spp)
_case("samples", "spp_65536", "default", None, 2, 2, 65536)

_case("sphere_ids", "spheres_65534", ("many", 65534), None, 16, 16, 2)
_case("sphere_ids", "spheres_65535", ("many", 65535), None, 16, 16, 2)

for _w, _h in ((8, 65535), (65535, 8), (8, 65536), (65536, 8), (2, 32768)):
    _case("extents", "frame_%dx%d" % (_w, _h), "default", TALL_CAMERA, _w, _h, 1)

for _w, _h in ((2, 8192), (8192, 2)):
    for _n in (32, 31, 33):
        _case("batched", "batch_%dx%d_x%d" % (_w, _h, _n), "default", TALL_CAMERA, _w, _h, 1, 0, _n, "batch", [32, 1] if _n == 33 else [_n])
_case("batched", "clip_2x8192_x32", "default", TALL_CAMERA, 2, 8192, 1, 0, 32, "camera_clip", [32])

FRAME_NUMBERS = {"2^24-1": 2 ** 24 - 1, "2^24": 2 ** 24, "2^24+1": 2 ** 24 + 1, "2^31-2": 2 ** 31 - 2}
for _name, _f in FRAME_NUMBERS.items():
    _case("frame_numbers", "frame_" + _name, "default", None, 24, 16, 2, _f)
for _name, _f in (("2^24-1", 2 ** 24 - 1), ("2^31-4", 2 ** 31 - 4)):
    _case("frame_numbers", "batch3_from_" + _name, "default", None, 24, 16, 2, _f, 3, "batch", [3])
    _case("frame_numbers", "moments3_from_" + _name, "default", None, 24, 16, 2, _f, 3, "batch_moments", [3])
_case("frame_numbers", "frame_2^31-2_alone", "default", None, 24, 16, 2, 2 ** 31 - 2, flags=0)
_case("frame_numbers", "batch3_from_2^31-4_alone", "default", None, 24, 16, 2, 2 ** 31 - 4, 3, "batch", [3], flags=0)
_case("frame_numbers", "moments3_from_2^31-4_alone", "default", None, 24, 16, 2, 2 ** 31 - 4, 3, "batch_moments", [3], flags=0)

FAMILIES = {f: tuple(n for n in CASES if FAMILY_OF[n] == f) for f in dict.fromkeys(FAMILY_OF.values())}
# the values at a seam, which the GPU tests also run on the other kernel variants: the last value of the path-queue kernel and the first
# of the lane-refill kernel
SEAM_PAIRS = (("spp_2047", "spp_2048"), ("frame_8x65535", "frame_8x65536"), ("frame_65535x8", "frame_65536x8"))


def build(name):
    """-> (spheres, mats, camera, w, h, spp, first_frame, frames)"""
    key, camera, w, h, spp, first_frame, frames = CASES[name]
    s, m = scene(key)
    return s, m, (None if camera is None else dict(camera)), w, h, spp, first_frame, frames


def path_queue_side(name):
    """whether a context set up for the path-queue kernel traces this case's frames with it (the table above)"""
    s, _, _, w, h, spp, _, _ = build(name)
    return spp <= MAX_SPP and len(s) <= MAX_SPHERES and w <= MAX_EXTENT and h <= MAX_EXTENT
