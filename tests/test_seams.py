"""The catalogue of tests/seams_lib.py on the CPU, at the sizes tests/test_gpu_seams.py draws it on the GPU: every case is what its name
says.  The oracle renders each case once (wanted(): shared with the GPU file); its image is finite, not of one colour, and its paths hit
the scene.  The many-sphere scenes show every planted index to the camera, a glass and a metal sphere with an id of 32640 or more among
them (their bounce rays carry that id through the path record), and are grouped by buildGroups.  The tall frames have spheres, not sky,
in the rows whose pixel words are NaN bit patterns.  The table of seams_lib's docstring is held as arithmetic: the three packings
round-trip over the catalogue's extents, the NaN-pattern ranges are exactly the ones it names, and the catalogue reaches into each.  And
the host's side of every seam -- which kernel tptDrawDevice takes at the limit and past it, what the other entry points refuse -- is held
on the emulated runtime (tests/hostemu), where the two kernels show in the LDS size of the recorded launch."""
import ctypes as C

import numpy as np
import pytest

import seams_lib as lib
from batch_moments_lib import blend, lerp_factor
from common import oracle_frames
from isa_lib import run_refusals
from moments_lib import MomentsChecker
from object_lib import ObjectChecker, centre_rays, object_plane_numpy
from oracle_lib import FLAG_PROGRESSIVE, SEED_PER_PIXEL
from test_scene_kinds import group_info

_wanted = {}


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """the existing modules' CPU statements of the planes, built on first use and once"""
    built = {}

    def get(cls):
        if cls not in built:
            built[cls] = cls(tmp_path_factory.mktemp(cls.__name__))
        return built[cls]
    return get


def previous(name):
    """the tile a case's frames are blended into: finite and non-zero where the frame number is the subject, zeroed elsewhere"""
    _, _, _, w, h, _, _, _ = lib.build(name)
    return lib.previous_tile(w, h) if lib.FAMILY_OF[name] == "frame_numbers" else np.zeros((h, w, 4), np.float32)


def wanted(oracle, name, checkers=None):
    """what the device must render of a case, computed once per process and left as it is -> dict: `tile` (the image after the last
    frame), `rays` (per frame); for the entries with planes (batch_moments, camera_clip; they need `checkers`) also `moments`, `albedo`,
    `nd` as the call leaves them and, for the clip, the per-frame planes `images`, `fmo`, `f_albedo`, `f_nd`"""
    if name in _wanted:
        return _wanted[name]
    s, m, camera, w, h, spp, first, frames = lib.build(name)
    cam = lib.oracle_camera(oracle, camera, w, h)
    entry, flags = lib.ENTRY[name], lib.FLAGS[name]
    if entry in ("draw", "batch"):
        _, tile, per = oracle_frames(oracle, w, h, spp, frames, flags, spheres=s, mats=m, cam=cam, seed_mode=SEED_PER_PIXEL, first=first,
                                     bb=previous(name))
        out = dict(tile=tile, rays=per)
    else:
        checker = checkers(MomentsChecker)
        tile, mo = previous(name), lib.previous_tile(w, h, seed=8)
        alb, nd = lib.previous_tile(w, h, seed=9), lib.previous_tile(w, h, seed=10)
        out = dict(rays=[], images=[], fmo=[], f_albedo=[], f_nd=[])
        for f in range(first, first + frames):
            r, _, _, a, n = checker.render(s, m, cam, w, h, spp, f, flags, backbuffer=tile, moments=mo)
            out["rays"].append(r)
            if entry == "camera_clip":
                for k, v in (("images", tile.copy()), ("fmo", mo.copy()), ("f_albedo", a), ("f_nd", n)):
                    out[k].append(v)
            else:  # (tptDrawDeviceBatchMoments blends the guides as it blends the tile: include/tpt_hip.h)
                blend(alb, a, lerp_factor(f, flags))
                blend(nd, n, lerp_factor(f, flags))
        out.update(tile=tile, moments=mo, albedo=alb, nd=nd)
    for v in out.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    _wanted[name] = out
    return out


def start_planes(name):
    """the four planes a batch_moments / camera_clip case starts from, as wanted() does: (tile, moments, albedo, normal / depth)"""
    _, _, _, w, h, _, _, _ = lib.build(name)
    return previous(name), lib.previous_tile(w, h, seed=8), lib.previous_tile(w, h, seed=9), lib.previous_tile(w, h, seed=10)


def first_hit_plane(oracle, checkers, name):
    """the sphere the ray through each pixel's centre hits first (-1: the sky) -> int32 [h, w]; tests/object_checker.c up to 8192 x 8192,
    its numpy twin beyond"""
    s, m, camera, w, h, _, _, _ = lib.build(name)
    cam = lib.oracle_camera(oracle, camera, w, h)
    if max(w, h) <= 8192:
        return checkers(ObjectChecker).plane(s, cam, w, h)[0]
    return object_plane_numpy(s, cam, w, h)


# ---------------------------------------------------------------- 1. every case: finite, not of one colour, and its paths hit the scene
@pytest.mark.parametrize("name", list(lib.CASES))
def test_the_oracle_renders_something_to_compare(oracle, checkers, name):
    _, _, _, w, h, spp, _, frames = lib.build(name)
    want = wanted(oracle, name, checkers)
    tile = want["tile"]
    assert np.isfinite(tile).all(), "the oracle's own image is not finite: the case is no fair test (tests/seams_lib.py)"
    colours = tile[..., :3].reshape(-1, 3)
    assert (colours != colours[0]).any(), "every pixel has one colour"
    assert len(want["rays"]) == frames
    assert sum(want["rays"]) > w * h * spp * frames, "no path of the case hits anything: rays per primary ray is 1"


def test_the_previous_tile_shows_in_the_frame_number_cases(oracle, checkers):
    """lerpFac = float(f) / float(f + 1) is 1 - 2^-24 at f = 2^24 - 1 and exactly 1 at 2^24 (2^24 + 1 is no binary32 number), below 1
    once more at 2^24 + 1, and 1 for every frame from 2^25 on: a frame blended with 1 leaves the tile what it was, to the last bit, and
    on a zeroed tile nothing of that would show.  The cases therefore start from a tile that is not zero, and the oracle's result is
    never the frame alone; it is the previous tile exactly where every frame's factor is 1."""
    one = np.float32(1)
    frames = (2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 4, 2 ** 31 - 2)
    assert [lerp_factor(f, FLAG_PROGRESSIVE) == one for f in frames] == [False, True, False, True, True]
    for name in lib.FAMILIES["frame_numbers"]:
        s, m, camera, w, h, spp, first, frames = lib.build(name)
        tile = wanted(oracle, name, checkers)["tile"]
        _, alone, _ = oracle_frames(oracle, w, h, spp, 1, 0, spheres=s, mats=m, seed_mode=SEED_PER_PIXEL, first=first + frames - 1)
        kept = all(lerp_factor(f, lib.FLAGS[name]) == one for f in range(first, first + frames))
        assert (tile[..., :3].tobytes() == previous(name)[..., :3].tobytes()) == kept, name
        # without the progressive flag the tile is the last frame alone: what shows the seeds of the frames whose factor is 1
        assert (tile[..., :3].tobytes() == alone[..., :3].tobytes()) == (lib.FLAGS[name] == 0), name


# ---------------------------------------------------------------- 2. the many-sphere scenes
@pytest.mark.parametrize("name", lib.FAMILIES["sphere_ids"])
def test_every_planted_index_is_seen_and_large_ids_bounce(oracle, checkers, emu, name):
    s, m, camera, w, h, _, _, _ = lib.build(name)
    n = len(s)
    planted = lib.planted(n)
    assert n == (65534 if name == "spheres_65534" else 65535) and max(planted) == n - 1
    s0, m0 = oracle.default_scene()
    for at, i in planted.items():
        assert s[at].tobytes() == s0[i].tobytes() and m[at].tobytes() == m0[i].tobytes()
    plane = first_hit_plane(oracle, checkers, name)
    # the object plane is HitSpheres on the rays through the pixel centres: the oracle's own says the same
    o, d = centre_rays(lib.oracle_camera(oracle, camera, w, h), w, h)
    o, t = np.ascontiguousarray(o, np.float32), C.c_float()
    for y in range(h):
        for x in range(w):
            ray = np.float32([d[0][y, x], d[1][y, x], d[2][y, x]])
            assert oracle.lib.tpto_hit_spheres(s.ctypes.data, n, o.ctypes.data, ray.ctypes.data, 0.001, 1.0e7, C.byref(t), None, None) == plane[y, x]
    seen = set(np.unique(plane).tolist())
    assert set(planted) <= seen, "planted indices the camera's rays never hit first: %s" % sorted(set(planted) - seen)
    for ids in lib.NAN_SPHERE_IDS:  # a hit id in each range whose record word is a NaN pattern
        assert seen & set(ids), ids
    # a bounce ray leaves a sphere with an id of 32640 or more: glass always scatters, a mirror of roughness 0 reflects what reaches it
    glass = [i for i in seen if i >= 32640 and m["type"][i] == lib.DIELECTRIC]
    mirror = [i for i in seen if i >= 32640 and m["type"][i] == lib.METAL and m["roughness"][i] == 0]
    assert 32640 in glass and mirror, (glass, mirror)
    groups, _, big = group_info(emu, s, m)
    assert groups > 0 and big <= 64, (groups, big)


def test_the_two_many_sphere_scenes_differ_by_one_sphere():
    a, b = lib.build("spheres_65534")[0], lib.build("spheres_65535")[0]
    assert len(a) == lib.MAX_SPHERES and len(b) == lib.MAX_SPHERES + 1
    assert lib.path_queue_side("spheres_65534") and not lib.path_queue_side("spheres_65535")


# ---------------------------------------------------------------- 3. spheres, not sky, in the rows whose words are NaN patterns
def test_the_nan_pattern_rows_of_the_tall_frames_show_the_scene(oracle, checkers):
    cases = [("frame_8x65535", lib.NAN_ROWS_SINGLE), ("frame_8x65536", lib.NAN_ROWS_SINGLE), ("frame_2x32768", lib.NAN_ROWS_SINGLE[:1])]
    cases += [(n, (lib.NAN_ROWS_BATCH_SLOT_31,)) for n in lib.FAMILIES["batched"] if "2x8192" in n]
    for name, bands in cases:
        s, m, camera, w, h, spp, first, frames = lib.build(name)
        plane = first_hit_plane(oracle, checkers, name)
        for rows in bands:
            rows = [y for y in rows if y < h]
            assert rows and (plane[rows] >= 0).all(), (name, rows[0], "the band shows sky")
            assert len(np.unique(wanted(oracle, name, checkers)["tile"][rows][..., :3].reshape(-1, 3), axis=0)) > len(rows), (name, "a flat band")
        if lib.ENTRY[name] != "draw" and frames >= 32:
            # slot 31 of the launch: the frame alone (lerpFac = 0 without the progressive flag) differs from the sky's gradient there
            cam = lib.oracle_camera(oracle, camera, w, h)
            _, alone = oracle.render(s, m, cam, w, h, spp, first + 31, 0, seed_mode=SEED_PER_PIXEL)
            band = alone[list(lib.NAN_ROWS_BATCH_SLOT_31)][..., :3]
            assert np.isfinite(band).all() and len(np.unique(band.reshape(-1, 3), axis=0)) > 1000, name


# ---------------------------------------------------------------- 4. the table, as arithmetic
def test_the_packings_round_trip_over_the_catalogues_extents():
    rng = np.random.default_rng(1)
    for name in lib.CASES:
        s, _, _, w, h, spp, first, frames = lib.build(name)
        if not lib.path_queue_side(name):
            continue  # (the lane-refill kernel packs nothing)
        xs = np.unique(np.concatenate([[0, w - 1], rng.integers(0, w, 64)]))
        ys = np.arange(h)
        px, py = np.meshgrid(xs, ys)
        if name in lib.LAUNCHES and max(lib.LAUNCHES[name]) > 1:
            assert w <= lib.MAX_BATCH_EXTENT and h <= lib.MAX_BATCH_EXTENT and max(lib.LAUNCHES[name]) <= lib.MAX_BATCH
            for slot in {0, max(lib.LAUNCHES[name]) - 1}:
                x, y, f = lib.unpack_batch_pixel(lib.pack_batch_pixel(px, py, slot))
                assert (x == px).all() and (y == py).all() and (f == slot).all(), name
        else:
            x, y = lib.unpack_pixel(lib.pack_pixel(px, py))
            assert (x == px).all() and (y == py).all(), name
        ids = np.concatenate([[-1], np.arange(len(s))])
        for sample in {0, spp - 1}:
            for depth, e in ((0, 1), (10, 0)):
                sm, dp, de, rid = lib.unpack_record(lib.pack_record(sample, depth, e, ids))
                assert (sm == sample).all() and (dp == depth).all() and (de == e).all() and (rid == ids).all(), name
    # one past each limit does not: what the host routes by
    assert lib.unpack_record(lib.pack_record(2048, 0, 1, 0))[0] != 2048
    assert lib.unpack_record(lib.pack_record(0, 0, 1, 65535))[3] == -1  # (the 65536th sphere's id reads as "no hit")
    assert lib.unpack_pixel(lib.pack_pixel(0, 65536))[1] != 65536 and lib.unpack_pixel(lib.pack_pixel(65536, 0))[1] != 0
    assert lib.unpack_batch_pixel(lib.pack_batch_pixel(8192, 0, 0))[1] != 0 and lib.unpack_batch_pixel(lib.pack_batch_pixel(0, 8192, 0))[2] != 0


def _ranges(values):
    """sorted ints -> the list of ranges they form"""
    out, values = [], sorted(values)
    for v in values:
        if out and v == out[-1][-1] + 1:
            out[-1] = range(out[-1][0], v + 1)
        else:
            out.append(range(v, v + 1))
    return out


def test_the_nan_pattern_ranges_are_the_ones_the_table_names():
    """a value of the upper field is listed when its word is a NaN pattern for some value of the fields below it"""
    low = np.uint32([0, 1, 7, 0x1fff, 0xffff])
    rows = np.arange(65536, dtype=np.uint32)
    nan = lib.is_nan_pattern(lib.pack_pixel(low[None, :], rows[:, None])).any(axis=1)
    assert _ranges(np.nonzero(nan)[0].tolist()) == list(lib.NAN_ROWS_SINGLE)
    assert lib.is_signalling(lib.pack_pixel(1, 32640)) and not lib.is_signalling(lib.pack_pixel(1, 32704))
    assert not lib.is_nan_pattern(lib.pack_pixel(0, 32640))  # (the bits of +infinity)
    rows, slots = np.arange(8192, dtype=np.uint32), np.arange(lib.MAX_BATCH, dtype=np.uint32)
    nan = lib.is_nan_pattern(lib.pack_batch_pixel(low[None, None, :4], rows[None, :, None], slots[:, None, None])).any(axis=2)
    assert np.nonzero(nan.any(axis=1))[0].tolist() == [31], "slot 31, and only that one"
    assert _ranges(np.nonzero(nan[31])[0].tolist()) == [lib.NAN_ROWS_BATCH_SLOT_31]
    ids = np.arange(65536, dtype=np.uint32)
    nan = np.zeros(65536, bool)
    for sample in (0, 1, 2046):
        for depth in (0, 10):
            for e in (0, 1):
                nan |= lib.is_nan_pattern(lib.pack_record(sample, depth, e, ids))
    assert _ranges(np.nonzero(nan)[0].tolist()) == list(lib.NAN_SPHERE_IDS)
    assert lib.is_signalling(lib.pack_record(0, 0, 1, 32640)) and not lib.is_signalling(lib.pack_record(0, 0, 1, 32704))
    assert lib.is_nan_pattern(lib.pack_record(3, 2, 1, -1)), "no hit (0xffff), the one pattern the suite rendered before"


def test_the_catalogue_reaches_into_every_nan_pattern_range(oracle, checkers):
    """a rendered pixel of a path-queue case in each range of rows, a first hit in each range of ids (test 2 above holds the ids)"""
    single = [n for n in lib.FAMILIES["extents"] if lib.path_queue_side(n)]
    for rows in lib.NAN_ROWS_SINGLE:
        assert any(lib.build(n)[4] > rows[0] and lib.build(n)[3] > 1 for n in single), rows
    assert any(lib.build(n)[4] > max(lib.NAN_ROWS_SINGLE[0]) for n in single)  # (the whole first range: 32640 .. 32767)
    pools = [n for n in lib.FAMILIES["batched"] if lib.ENTRY[n] == "batch" and 32 in lib.LAUNCHES[n] and lib.build(n)[4] == 8192]
    clips = [n for n in lib.FAMILIES["batched"] if lib.ENTRY[n] == "camera_clip" and 32 in lib.LAUNCHES[n] and lib.build(n)[4] == 8192]
    assert pools and clips, "slot 31 with rows 7168 .. 8191: on the frame-pools kernel and on the clip kernel"
    for ids in lib.NAN_SPHERE_IDS:
        assert set(ids) & set(lib.planted(lib.MAX_SPHERES))
    assert {lib.build(n)[5] for n in lib.FAMILIES["samples"]} >= {17, 1024, 2046, 2047, 2048, 2049, 65536}
    assert {lib.build(n)[6] for n in lib.FAMILIES["frame_numbers"]} >= {2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 2, 2 ** 31 - 4}
    assert max(lib.build(n)[6] + lib.build(n)[7] - 1 for n in lib.CASES) == 2 ** 31 - 2  # (2^31 - 1 stays out: seams_lib's docstring)


# ---------------------------------------------------------------- 5. the host's side of every seam, on the emulated runtime
ROUTING = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from toypathtracer_amd import api as tpt
import seams_lib as lib
from common import oracle_frames
from oracle_lib import FLAG_PROGRESSIVE, SEED_PER_PIXEL, Oracle
o = Oracle.get()
QUEUES, REFILL = (0, 3, -1), (0, 1, -1)
tpt.InitializeTest()
def reset(spp=4, scene=None, variant=QUEUES):
    tpt.set_seed_mode(1); tpt.set_fold_mode(0); tpt.set_kernel_variant(*variant); tpt.set_samples_per_pixel(spp)
    tpt.set_camera(None)
    tpt.set_scene(*scene) if scene is not None else tpt.set_scene(None)
def plain(w, h, spp=1, scene=None, variant=QUEUES):
    """one frame through tptDrawDevice, held against the oracle -> the LDS bytes of its launch"""
    reset(spp, scene, variant)
    tile = np.zeros((h, w, 4), np.float32)
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    r0 = tpt.ray_counter_read()
    tpt.draw_device(0.0, 0, w, h, tile.ctypes.data, FLAG_PROGRESSIVE)
    tpt.synchronize()
    rays = tpt.ray_counter_read() - r0
    kw = dict(spheres=scene[0], mats=scene[1]) if scene is not None else {}
    total, want, _ = oracle_frames(o, w, h, spp, 1, seed_mode=SEED_PER_PIXEL, **kw)
    assert rays == total and tile.tobytes() == want.tobytes(), (w, h, spp, variant)
    return tpt.launch_info()["lds_bytes"]
def seam(what, at, past):
    """at the limit the context's own kernel, another one than the lane-refill kernel's launch; past it the lane-refill kernel's"""
    a, a_refill, p, p_refill = plain(**at), plain(variant=REFILL, **at), plain(**past), plain(variant=REFILL, **past)
    assert a != a_refill, (what, "at the limit the lane-refill kernel ran", a, a_refill)
    assert p == p_refill, (what, "past the limit the path-queue kernel ran", p, p_refill)
    print("routed:", what, "--", a, a_refill, p, p_refill)
seam("2047 | 2048 spp", dict(w=1, h=1, spp=2047), dict(w=1, h=1, spp=2048))
seam("65535 | 65536 columns", dict(w=65535, h=1), dict(w=65536, h=1))
seam("65535 | 65536 rows", dict(w=1, h=65535), dict(w=1, h=65536))
s34, s35 = lib.build("spheres_65534")[:2], lib.build("spheres_65535")[:2]
seam("65534 | 65535 spheres", dict(w=4, h=4, scene=s34), dict(w=4, h=4, scene=s35))

# ---- what the other entry points refuse past a limit (the sides no other test holds)
w, h = 16, 8
planes = [np.full((h, w, 4), 2.5 + k, np.float32) for k in range(6)]
before = [p.copy() for p in planes]
p = [x.ctypes.data for x in planes]
views = np.float32([[0, 2, 3, 0, 0, 0, 60, 0.02, 3]] * 2)
two = np.zeros((2, h, w, 4), np.float32)
times = np.float32([0.0, 0.0])
counts = np.full((h, w), 2, np.int32)
def refused(what, expect, call):
    try:
        call()
    except tpt.TptError as e:
        assert all(x in str(e) for x in expect), (what, str(e))
        print("refused:", what, "--", e)
        return
    raise AssertionError("%s was accepted" % what)
def entries():
    return {
        "tptDrawDeviceBatch": lambda: tpt.draw_device_batch(0.0, 0, 2, w, h, p[0], FLAG_PROGRESSIVE),
        "tptDrawDeviceViews": lambda: tpt.draw_device_views(0.0, 0, w, h, views, two.ctypes.data, FLAG_PROGRESSIVE),
        "tptDrawDeviceAov": lambda: tpt.draw_device_aov(0.0, 0, w, h, p[0], FLAG_PROGRESSIVE, albedo_ptr=p[2], normal_depth_ptr=p[3]),
        "tptDrawDeviceMoments": lambda: tpt.draw_device_moments(0.0, 0, w, h, p[0], p[1], FLAG_PROGRESSIVE, albedo_ptr=p[2], normal_depth_ptr=p[3]),
        "tptDrawDeviceAdaptive": lambda: tpt.draw_device_adaptive(0.0, 0, w, h, p[0], p[1], counts.ctypes.data, FLAG_PROGRESSIVE),
        "tptDrawDeviceAnimationMoments": lambda: tpt.draw_device_animation_moments(times, 0, w, h, p[0], p[1], FLAG_PROGRESSIVE),
        "tptDrawDeviceCameraClip": lambda: tpt.draw_device_camera_clip(times, views, 0, w, h, p[0], p[1], FLAG_PROGRESSIVE),
    }
QUEUE = "needs the path-queue kernel"
reset(spp=2048)
tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
refused("2048 spp, tptDrawDeviceBatch", ["tptDrawDeviceBatch", QUEUE], entries()["tptDrawDeviceBatch"])
refused("2048 spp, tptDrawDeviceViews", ["tptDrawDeviceViews", QUEUE, "at most 2047 spp"], entries()["tptDrawDeviceViews"])
reset(scene=s35)
tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
for fn, expect in (("tptDrawDeviceBatch", ["tptDrawDeviceBatch", QUEUE]), ("tptDrawDeviceViews", ["tptDrawDeviceViews", QUEUE]),
                   # (the planes' entry points share one message, which speaks of tptDrawDeviceAov)
                   ("tptDrawDeviceAov", ["tptDrawDeviceAov", QUEUE]), ("tptDrawDeviceMoments", [QUEUE]), ("tptDrawDeviceAdaptive", [QUEUE]),
                   ("tptDrawDeviceAnimationMoments", ["tptDrawDeviceAnimationMoments", "at most 65534 spheres"]),
                   ("tptDrawDeviceCameraClip", ["tptDrawDeviceCameraClip", "at most 65534 spheres"])):
    refused("65535 spheres, " + fn, expect, entries()[fn])
reset()
for ww, hh in ((8193, 2), (2, 8193)):
    tile = np.full((hh, ww, 4), 1.5, np.float32)
    tpt.UpdateTest(0.0, 0, ww, hh, FLAG_PROGRESSIVE)
    refused("tptDrawDeviceBatch, %d x %d" % (ww, hh), ["tptDrawDeviceBatch", "8192 x 8192"],
            lambda: tpt.draw_device_batch(0.0, 0, 2, ww, hh, tile.ctypes.data, FLAG_PROGRESSIVE))
    tpt.synchronize()
    assert (tile == 1.5).all()
    tile[...] = 0.0
    tpt.draw_device_batch(0.0, 0, 1, ww, hh, tile.ctypes.data, FLAG_PROGRESSIVE)  # (a batch of one is a plain frame, of any size)
    tpt.synchronize()
    assert tile.tobytes() == oracle_frames(o, ww, hh, 4, 1, seed_mode=SEED_PER_PIXEL)[1].tobytes()
tpt.synchronize()
assert all(a.tobytes() == b.tobytes() for a, b in zip(planes, before)) and not two.any(), "a refused call wrote"
# at the limits the same entry points pass their checks (what the emulated runtime has kernels for: the plain batch)
reset(spp=2047)
tile = np.zeros((1, 1, 4), np.float32)
tpt.UpdateTest(0.0, 0, 1, 1, FLAG_PROGRESSIVE)
tpt.draw_device_batch(0.0, 0, 2, 1, 1, tile.ctypes.data, FLAG_PROGRESSIVE)
tpt.synchronize()
assert tile.tobytes() == oracle_frames(o, 1, 1, 2047, 2, seed_mode=SEED_PER_PIXEL)[1].tobytes()
reset()
tpt.ShutdownTest()
print("ok")
'''


def test_the_host_routes_and_refuses_at_the_limits():
    # (the build with tptDrawDeviceAdaptive's blend, which tests/test_adaptive_abi.py makes too)
    out = run_refusals(ROUTING, "libtpt_hostemu_adaptive.so", ["hostemu_adaptive.cpp"])
    assert out.count("routed:") == 4, out
    assert out.count("refused:") == 2 + 7 + 2, out
