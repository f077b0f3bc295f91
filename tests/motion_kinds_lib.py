"""TEST INFRASTRUCTURE: clips whose MOTION is the subject, for tests/test_motion_kinds.py (the oracle, the host restatement of the trace
code and the emulated host runtime, on the CPU) and tests/test_gpu_motion_kinds.py (the moved-sphere kernels on the GPU).  One launch of
tptDrawDeviceKeyframeClip, tptDrawDeviceCameraClip, tptDrawDeviceAnimation and tptDrawDeviceAnimationMoments stages the scene of its LAST
frame: the packed pairs, the binary16 matrix table and the light flags are that scene's, and frames 0 .. n - 2 read the moved spheres'
centres from a table in LDS (tpt_trace.h, movedSphere / keyedSphere).  The rest of the suite moves spheres by +-0.3; here a sphere crosses
the table's limit, lands on another sphere, swallows the camera, a light leaves the scene or sits on the floor, the ground goes away.

A keyframe case is a builder that returns (spheres, materials, views[n, 9], ids[K], centres[n, K, 3], flags, first): what
tptDrawDeviceKeyframeClip takes, over scenes of tests/scene_kinds_lib.py wherever one exists.  CATALOGUE maps a name (the test id) to its
builder, FAMILIES a family to its names, META a name to what tests/test_motion_kinds.py proves of it:

  size            (w, h, spp): 96 x 54 x 2 as scene_kinds_lib.size_of, three frames, unless the case says otherwise
  light_sampling  False: the case runs with tptSetConfig(lightSampling = 0)
  table           per frame, whether packScene(S_j) builds a matrix table (the table_seam family)
  tie             (frame, shown, hidden): in that frame sphere `hidden` is exactly coincident with sphere `shown` < `hidden`
  inside          (frame, id): the camera's origin lies strictly inside that sphere in that frame only
  no_static       frames in which no static sphere fills 5 % of the view: the view stands beside a sphere 2^10 or more away, or the
                  camera is inside a moved sphere.  This list is WIDER than the one exemption that was asked for (the reach family
                  from 2^10 on): it also holds the 2^20 cases of the ids family, the frame of lights_far that looks at a far light,
                  and the camera-inside cases, for the same two reasons.  Every frame of every case shows a moved sphere.
  launches        the number of trace launches of one call (one per 32 frames; one per frame for the three fallbacks)

  reach        spheres 1 (Lambert), 4 (metal) and 7 (glass) moved by 2^k along x in the middle frame only (`_mid`: the staged scene is
               the scene at rest) or in the last frame only (`_last`: the staged scene is the far one), k = -20 ... 60; by one ulp; to
               +-3e38.  A far frame's view stands three to four units beside the moved spheres -- from 2^24 on, where binary32 has no
               such point along x, at the spheres' own x and beside them in y and z --: camera and bounce rays start outside the
               binary16 range of the matrix-core filter's ray operands, and from 2^40 on every camera ray has the origin's x and no
               x in its direction (the lens' horizontal extent is below one ulp of 2^40);
  table_seam   sphere 9 of scene_kinds_lib.big_sphere_at (r = 30) at x = 244, 244.9 (a table), 245, 300 (none) and at the two floats on
               either side of the limit (TABLE_SEAM, found by bisection on packScene's mxR1 by the test that builds the case): out of
               range in the last frame only, in an earlier frame only, alternating; the same with the small sphere 2 moving through
               the view, where the staged table's filter would drop it from most rays that hit it (`seam_small_sphere_in_in_the_last`); 33 frames
               whose two launches stage scenes of different kinds, sphere 1 rising a little per frame;
  ties         a moved sphere exactly on a static one of lower / higher index, two moved spheres on each other, a moved sphere inside
               a static glass one, a moved glass shell around a static mirror, the camera inside a moved sphere, the ground +-100 in y;
  lights       both emissive spheres (8 and 45) 2^20 away, coincident, centred on the floor, and moved a little while sphere 2 passes
               between them and the floor; all of it again without light sampling (`_nols`);
  degenerate   a moved zero radius, a moved negated radius, the same centres in consecutive frames, eight spheres "moved" to their
               own centres, centres with -0.0 components;
  ids          K = 1 ... 8 moved spheres; sphere 0 alone, sphere 63 alone in a 64-sphere scene, {0, 63} in flat scenes of 65, 128 and
               255 spheres, each by 2^7 and 2^20; the three calls that go frame by frame (nine moved spheres, an id of 64, 256 spheres).

TIMED holds the clips of the three time-driven calls (spheres 1 and 8 move by cos t + 1 and 0.3 sin t): (spheres, materials, times, views,
flags, first) over scenes whose sphere 1 or 8 is emissive, glass around the camera, coincident with a static sphere, or across the table's
limit at one of the times; the times are searched for on the CPU by the builder and asserted by tests/test_motion_kinds.py.

Nothing under toypathtracer_amd/ imports this module."""
import math

import numpy as np

import scene_kinds_lib as kinds
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE
from scene_kinds_lib import DEFAULT_CAMERA, DIELECTRIC, LAMBERT, METAL

f32 = np.float32
SIZE = (96, 54, 2)
HOME = tuple(DEFAULT_CAMERA["look_from"]) + tuple(DEFAULT_CAMERA["look_at"]) + (DEFAULT_CAMERA["vfov"], DEFAULT_CAMERA["aperture"],
                                                                              DEFAULT_CAMERA["focus_dist"])
REACH_IDS = (1, 4, 7)  # Lambert, metal, glass
LIGHTS = (8, 45)
TABLE_SEAM = None  # (last x with a table, first x without) for sphere 9 of big_sphere_at: set_table_seam()


def set_table_seam(inside, outside):
    """what the bisection on packScene(...).mxR1 found (tests/test_motion_kinds.py table_seam_of): adjacent floats"""
    global TABLE_SEAM
    assert f32(inside) < f32(outside) and np.nextafter(f32(inside), f32(np.inf)) == f32(outside)
    TABLE_SEAM = (f32(inside), f32(outside))


def view(look_from, look_at, vfov=60.0, aperture=0.02, focus=None):
    o, a = [float(f32(v)) for v in look_from], [float(f32(v)) for v in look_at]
    if focus is None:
        focus = float(f32(math.dist(o, a)))
    return tuple(o) + tuple(a) + (float(vfov), float(aperture), float(focus))


def beside(centre, radius=0.5, side=(1.0, 0.35, 0.2), distance=3.0, fill=0.25):
    """a view of the sphere from `distance` (about 3 units, more for a big sphere) beside it, on the side away from the origin for a sphere
    moved along +x, looking back through it at where it came from; the lens is chosen so that the sphere's radius spans `fill` of the
    image height"""
    n = math.sqrt(sum(v * v for v in side))
    d = max(distance, 3.2 * abs(radius))
    o = [float(f32(c) + f32(d * v / n)) for c, v in zip(centre, side)]
    dist = math.dist(o, [float(f32(c)) for c in centre])
    vfov = 2.0 * math.degrees(math.atan(abs(radius) / dist / (2.0 * fill)))
    return view(o, centre, vfov=min(vfov, 90.0))


def centres_of(s, ids, n):
    """the scene's own centres of `ids`, n times -> float32 (n, K, 3)"""
    base = np.stack([s["cx"][list(ids)], s["cy"][list(ids)], s["cz"][list(ids)]], axis=-1).astype(f32).reshape(len(ids), 3)
    return np.repeat(base[None], n, axis=0).copy()


def scene_of(spheres, ids, centres, j):
    """S_j: the spheres with the centres of the moved ids replaced by frame j's"""
    s = spheres.copy()
    for k, i in enumerate(ids):
        s["cx"][i], s["cy"][i], s["cz"][i] = centres[j, k]
    return s


def _case(s, m, views, ids, centres, flags=FLAG_PROGRESSIVE, first=0):
    views = np.asarray(views, f32).reshape(-1, 9)
    ids = np.asarray(ids, np.int32).reshape(-1)
    centres = np.ascontiguousarray(centres, f32).reshape(len(views), len(ids), 3)
    assert np.isfinite(centres).all() and np.isfinite(views).all()
    return s, m, views, ids, centres, flags, first


def _default():
    s, m, _ = kinds.scene("aperture_0")  # (the built-in scene; the camera is not the scene's)
    s, m = s.copy(), m.copy()
    assert m["type"][1] == LAMBERT and m["type"][4] == METAL and m["type"][7] == DIELECTRIC and m["type"][2] == LAMBERT
    assert [i for i in range(len(m)) if (m["emissive"][i] > 0).any()] == list(LIGHTS)
    return s, m


def _builtin(name):
    s, m, _ = kinds.scene(name)
    return s.copy(), m.copy()


META = {}
FAMILY_BUILDERS = {}


def _add(family, name, build, **meta):
    meta.setdefault("size", SIZE)
    meta.setdefault("light_sampling", True)
    meta.setdefault("no_static", ())
    meta["family"] = family
    assert name not in META, name
    META[name] = meta
    FAMILY_BUILDERS.setdefault(family, {})[name] = build


# ---------------------------------------------------------------- reach
def _reach_view(s, c):
    """the view of a far frame: beside the three moved spheres, which keep their places relative to each other"""
    mid = [float(np.mean(c[:, a])) for a in range(3)]
    if abs(mid[0]) >= 2.0 ** 23:  # (no binary32 point 3.5 beside them along x: the spheres' own x, beside them in y and z)
        return view((mid[0], 1.0, 4.0), (mid[0], 0.3, 0.0), vfov=50.0)
    return view((float(f32(mid[0]) + f32(3.5)), 1.6, 0.4), (mid[0], 0.3, 0.0), vfov=50.0)


def reach(delta, frame):
    """`delta(x)` -> the moved x; frame: the one frame of three in which the spheres are away"""
    def build():
        s, m = _default()
        c = centres_of(s, REACH_IDS, 3)
        c[frame, :, 0] = [delta(f32(x)) for x in c[frame, :, 0]]
        views = [HOME] * 3
        if float(np.abs(c[frame, :, 0] - centres_of(s, REACH_IDS, 1)[0, :, 0]).max()) >= 8.0:
            views[frame] = _reach_view(s, c[frame])
        return _case(s, m, views, REACH_IDS, c)
    return build


REACH_K = (-20, 0, 4, 7, 10, 20, 40, 60)
for _k in REACH_K:
    for _frame, _tag in ((1, "mid"), (2, "last")):
        _add("reach", "reach_2^%d_%s" % (_k, _tag), reach(lambda x, k=_k: f32(x + f32(2.0 ** k)), _frame), reach_k=_k,
             no_static=(_frame,) if _k >= 10 else ())
for _frame, _tag in ((1, "mid"), (2, "last")):
    _add("reach", "reach_1ulp_%s" % _tag, reach(lambda x: np.nextafter(f32(x), f32(np.inf)), _frame), reach_k=-24)


def reach_3e38():
    """the three spheres in three corners of binary32; the view stands at sphere 1's x, beside it in y and z"""
    s, m = _default()
    c = centres_of(s, REACH_IDS, 3)
    c[1] = [(3e38, 0.0, -1.0), (-3e38, 0.0, 1.0), (3e38, -3e38, 3e38)]
    return _case(s, m, [HOME, view((3e38, 0.5, 3.0), (3e38, 0.0, -1.0), vfov=40.0), HOME], REACH_IDS, c)


_add("reach", "reach_3e38", reach_3e38, reach_k=127, no_static=(1,))


# ---------------------------------------------------------------- table_seam
SEAM_ID = 9
SEAM_VIEW = view((-6.0, 0.5, 0.0), (244.0, 0.0, 0.0), vfov=24.0)


SEAM_SMALL = 2  # a sphere of r = 0.5 in front of the seam's camera
SEAM_SMALL_PATH = ((-2.0, 0.5, 0.375), (-1.0, 0.625, -0.375))  # where it is before it comes to rest at (0, 0, -1)


def table_seam(xs, also=None):
    """sphere 9 (r = 30) at xs[j] in frame j; a string names one side of TABLE_SEAM.  also = SEAM_SMALL: sphere 2 goes along
    SEAM_SMALL_PATH and is at rest in the last frame; also = 1: sphere 1 rises by 2^-6 per frame"""
    def build():
        s, m = _builtin("big_sphere_at_244")
        assert s["radius"][SEAM_ID] == 30
        x = [f32(v) if not isinstance(v, str) else TABLE_SEAM[("in", "out").index(v)] for v in xs]
        ids = [SEAM_ID] + ([also] if also is not None else [])
        c = centres_of(s, ids, len(x))
        c[:, 0, 0] = x
        if also == SEAM_SMALL:
            c[:len(SEAM_SMALL_PATH), 1] = SEAM_SMALL_PATH
        elif also == 1:
            c[:, 1, 1] += f32(2.0 ** -6) * np.arange(len(x), dtype=f32)
        return _case(s, m, [SEAM_VIEW] * len(x), ids, c)
    return build


IN, OUT = True, False
for _name, _xs, _table in (
        ("seam_out_in_the_last", (244, 244.9, 245), (IN, IN, OUT)),
        ("seam_out_in_the_first", (300, 244, 244.9), (OUT, IN, IN)),
        ("seam_out_in_the_middle", (244.9, 245, 244), (IN, OUT, IN)),
        ("seam_in_in_the_middle", (245, 244.9, 300), (OUT, IN, OUT)),
        ("seam_exact_out_in_the_last", ("in", "in", "out"), (IN, IN, OUT)),
        ("seam_exact_out_in_the_first", ("out", "in", "in"), (OUT, IN, IN)),
        ("seam_exact_out_in_the_middle", ("in", "out", "in"), (IN, OUT, IN)),
        ("seam_exact_in_in_the_middle", ("out", "in", "out"), (OUT, IN, OUT))):
    _add("table_seam", _name, table_seam(_xs), table=_table)
# the staged scene has a table and sphere 2 at rest: the table's filter alone would drop sphere 2 from the earlier frames' rays
_add("table_seam", "seam_small_sphere_in_in_the_last", table_seam((245, "out", 244.9), SEAM_SMALL), table=(OUT, OUT, IN))
# 33 frames: two launches (frames 0 .. 31 and frame 32), the first stages frame 31's scene (a table), the second frame 32's (none)
_X33 = tuple((244.9, "out", "in", 245)[j % 4] for j in range(31)) + ("in", "out")
_add("table_seam", "seam_33_frames", table_seam(_X33, 1), size=(48, 27, 1), launches=2,
     table=tuple((v == "in") if isinstance(v, str) else v < 245 for v in _X33))


# ---------------------------------------------------------------- ties
TIE_GROUND = f32(-100.5) - f32(2.0 ** -10)  # (the ground rides along, a hair lower, so that a moved sphere is in view in the tie's frame)


def tie(moved, at, shown, hidden, scene=None):
    """frame 1: the spheres `moved` stand exactly at sphere `at`'s centre (or at the point `at`)"""
    def build():
        s, m = _default()
        ids = list(moved) + [0]
        c = centres_of(s, ids, 3)
        p = (s["cx"][at], s["cy"][at], s["cz"][at]) if isinstance(at, int) else at
        c[1, :len(moved)] = p
        c[1, -1, 1] = TIE_GROUND
        return _case(s, m, [HOME, beside(p, 0.5, side=(-0.6, 0.5, 1.0), fill=0.22), HOME], ids, c)
    return build


_add("ties", "tie_on_a_lower_static", tie([5], 2, 2, 5), tie=(1, 2, 5))
_add("ties", "tie_on_a_higher_static", tie([2], 5, 2, 5), tie=(1, 2, 5))
_add("ties", "tie_of_two_moved", tie([4, 1], (-0.5, 0.5, 2.0), 1, 4), tie=(1, 1, 4))


def inside_a_static_glass():
    """sphere 2 with half the radius, in frame 1 at the centre of the glass sphere 7, in frame 2 a little off it"""
    s, m = _default()
    s["radius"][2] = f32(0.25)
    s["invRadius"][2] = f32(4)
    c = centres_of(s, [2, 0], 3)
    g = (s["cx"][7], s["cy"][7], s["cz"][7])
    c[1, 0] = g
    c[2, 0] = (g[0] + f32(0.125), g[1], g[2] - f32(0.0625))
    c[1:, 1, 1] = TIE_GROUND
    v = beside(g, 0.5, side=(-0.6, 0.5, 1.0), fill=0.22)
    return _case(s, m, [HOME, v, v], [2, 0], c)


def glass_shell_around_a_static_mirror():
    """scene_kinds_lib.glass_shell_around_a_mirror: sphere 46, the shell, stands above the mirror 3, then around it, then around it and off
    centre"""
    s, m = _builtin("glass_shell_around_a_mirror")
    c = centres_of(s, [46, 0], 3)
    c[0, 0, 1] += f32(2)
    c[2, 0, 0] += f32(0.125)
    c[1:, 1, 1] = TIE_GROUND
    v = beside((s["cx"][3], s["cy"][3], s["cz"][3]), 0.75, side=(-0.6, 0.5, 1.0), fill=0.22)
    return _case(s, m, [v, v, v], [46, 0], c)


_add("ties", "moved_inside_a_static_glass", inside_a_static_glass)
_add("ties", "glass_shell_around_a_static_mirror", glass_shell_around_a_static_mirror)


def camera_inside(i):
    def build():
        s, m = _default()
        c = centres_of(s, [i], 3)
        o = DEFAULT_CAMERA["look_from"]
        c[1, 0] = (o[0] + 0.125, o[1] - 0.0625, o[2] + 0.25)  # (the camera 0.29 from the centre of a sphere of radius 0.5)
        v = beside(c[0, 0], 0.5, side=(-0.6, 0.5, 1.0) if i != 4 else (0.8, 0.5, 1.0), fill=0.22)  # (at rest the sphere is seen from beside it)
        return _case(s, m, [v, HOME, v], [i], c)
    return build


for _name, _i in (("lambert", 1), ("metal", 4), ("glass", 7)):
    _add("ties", "camera_inside_a_moved_%s" % _name, camera_inside(_i), inside=(1, _i), no_static=(1,))

DOWN = view((0.0, 3.0, 3.0), (0.0, -1.0, 0.5), vfov=90.0)  # (looks down steeply: a ground 100 lower is still in view)


def ground_moved(dy):
    def build():
        s, m = _default()
        c = centres_of(s, [0], 3)
        c[1, 0, 1] += f32(dy)
        return _case(s, m, [HOME, DOWN, HOME], [0], c)
    return build


_add("ties", "ground_up_100", ground_moved(100.0), inside=(1, 0))  # (the camera is inside the ground, and so are the other spheres)
_add("ties", "ground_down_100", ground_moved(-100.0))


# ---------------------------------------------------------------- lights
def _floor_point(s, x, z):
    """the point of the ground sphere above (x, z), in binary32 as close as the square root gives it"""
    g = s[0]
    dx, dz = f32(x) - g["cx"], f32(z) - g["cz"]
    return (f32(x), f32(g["cy"] + np.sqrt(f32(g["radius"] * g["radius"] - dx * dx - dz * dz))), f32(z))


def lights_far():
    """frame 1: both lights 2^20 away, seen from home (the ground rides along, a hair lower: the shaded floor is what shows the
    light loop); frame 2: both 2^20 away along -z, the view beside light 8"""
    s, m = _default()
    ids = list(LIGHTS) + [0]
    c = centres_of(s, ids, 3)
    c[1, :2, 0] += f32(2.0 ** 20)
    c[2, :2, 2] -= f32(2.0 ** 20)
    c[1:, 2, 1] = TIE_GROUND
    return _case(s, m, [HOME, HOME, beside(c[2, 0], 0.3, side=(0.2, 0.3, -1.0))], ids, c)


def lights_coincident():
    """frame 1: light 45 on light 8; frame 2: both at a third place"""
    s, m = _default()
    ids = list(LIGHTS) + [0]
    c = centres_of(s, ids, 3)
    c[1, 1] = c[1, 0]
    c[2, :2] = (0.0, 1.5, 0.5)
    c[1:, 2, 1] = TIE_GROUND
    return _case(s, m, [HOME] * 3, ids, c)


def lights_on_the_floor():
    """both lights centred on points of the floor in front of the camera: the floor within 0.3 of either lies inside a light"""
    s, m = _default()
    ids = list(LIGHTS) + [0]
    c = centres_of(s, ids, 3)
    c[1, 0], c[1, 1] = _floor_point(s, -0.75, 1.75), _floor_point(s, 1.0, 1.5)
    c[2, 0], c[2, 1] = _floor_point(s, 0.0, 1.875), _floor_point(s, 0.0, 1.875)
    c[1:, 2, 1] = f32(-100.5)  # (the ground stays: the lights' centres are on it)
    return _case(s, m, [HOME] * 3, ids, c)


def lights_with_an_occluder():
    """both lights move a little while sphere 2 passes between them and the floor"""
    s, m = _default()
    ids = list(LIGHTS) + [2, 0]
    c = centres_of(s, ids, 3)
    for j, x in enumerate((-1.75, -1.25, 1.25)):
        c[j, 0] += f32(0.125) * f32(j - 1)
        c[j, 1, 1] -= f32(0.125) * f32(j)
        c[j, 2] = (x, 0.75, (0.0, 0.0, -2.0)[j])
    c[1:, 3, 1] = TIE_GROUND
    return _case(s, m, [HOME] * 3, ids, c)


for _name, _fn in (("lights_far", lights_far), ("lights_coincident", lights_coincident), ("lights_on_the_floor", lights_on_the_floor),
                   ("lights_with_an_occluder", lights_with_an_occluder)):
    _add("lights", _name, _fn, no_static=(2,) if _name == "lights_far" else ())
    _add("lights", _name + "_nols", _fn, light_sampling=False, no_static=(2,) if _name == "lights_far" else ())


# ---------------------------------------------------------------- degenerate
CLOSE = view((0.6, 1.0, 2.8), (0.0, 0.0, 0.0), vfov=55.0)  # (spheres 2, 5 and 7 large in view)


def moved_zero_radius():
    """scene_kinds_lib.zero_radius: sphere 5 has no surface wherever it goes; sphere 2 moves beside it"""
    s, m = _builtin("zero_radius")
    c = centres_of(s, [5, 2], 3)
    c[0, 1] = (-0.6, 0.125, 0.75)
    c[1] = [(0.25, 0.5, 1.5), (0.5, 0.25, 1.0)]
    c[2] = [(0.5, 1.0, 0.5), (-0.5, 0.125, 1.0)]  # (frame 2: the zero radius at the glass sphere's centre)
    return _case(s, m, [CLOSE] * 3, [5, 2], c)


def moved_negated_radius():
    s, m = _builtin("negated_radius_glass")
    assert s["radius"][7] < 0
    c = centres_of(s, [7], 3)
    c[1, 0] = (-0.5, 0.75, 1.0)
    c[2, 0] = (0.25, 0.5, 1.25)
    return _case(s, m, [CLOSE] * 3, [7], c)


def same_centres_twice():
    s, m = _default()
    c = centres_of(s, [2, 5, 7], 3)
    c[1] = [(0.5, 0.25, -0.5), (-0.75, 0.0, 1.25), (0.75, 0.75, 1.0)]
    c[2] = c[1]
    return _case(s, m, [CLOSE] * 3, [2, 5, 7], c)


OWN_IDS = (0, 45, 8, 2, 5, 7, 1, 4)


def own_centres():
    s, m = _default()
    return _case(s, m, [HOME, CLOSE, HOME], OWN_IDS, centres_of(s, OWN_IDS, 3))


def negative_zero():
    """spheres 2 and 5 stand at x = y = 0: the same places written with -0.0, and -0.0 in a coordinate that moves"""
    s, m = _default()
    c = centres_of(s, [2, 5], 3)
    c[1, :, 0] = f32(-0.0)
    c[1, :, 1] = f32(-0.0)
    c[2, 0] = (-0.0, 0.25, -0.0)
    c[2, 1] = (0.5, -0.0, -0.0)
    assert np.signbit(c[1, :, :2]).all()
    return _case(s, m, [CLOSE] * 3, [2, 5], c)


# (a zero radius is never seen; in frames 1 and 2 sphere 2 is the moved sphere in view)
_add("degenerate", "moved_zero_radius", moved_zero_radius)
_add("degenerate", "moved_negated_radius", moved_negated_radius)
_add("degenerate", "same_centres_twice", same_centres_twice)
_add("degenerate", "own_centres_of_eight", own_centres)
_add("degenerate", "negative_zero", negative_zero)


# ---------------------------------------------------------------- ids
K_IDS = (7, 0, 45, 1, 4, 2, 5, 8)


def k_moved(k):
    """the first k of K_IDS: frame 1 a seeded +-0.3 per axis, frame 2 another"""
    def build():
        s, m = _default()
        ids = K_IDS[:k]
        c = centres_of(s, ids, 3)
        rng = np.random.default_rng(100 + k)
        c[1:] += rng.uniform(-0.3, 0.3, (2, k, 3)).astype(f32)
        return _case(s, m, [CLOSE] * 3, ids, c)
    return build


for _k in range(1, 9):
    _add("ids", "moved_%d" % _k, k_moved(_k))


def _stress_views(n):
    from toypathtracer_amd.scenes import STRESS_CAMERA as c
    return [tuple(c["look_from"]) + tuple(c["look_at"]) + (c["vfov"], c["aperture"], c["focus_dist"])] * n


def ground_alone(k):
    """the built-in scene's ground 2^k along x in frame 1: from home the view follows it (k = 7), or stands above its top (k = 20)"""
    def build():
        s, m = _default()
        c = centres_of(s, [0], 3)
        c[1, 0, 0] += f32(2.0 ** k)
        v = view((-5.0, 1.5, 0.5), (128.0, -40.0, -1.0), vfov=70.0) if k == 7 else view((2.0 ** k + 3.0, 2.5, 2.0), (2.0 ** k, -0.5, -1.0))
        return _case(s, m, [HOME, v, HOME], [0], c)
    return build


def flat(n, ids, k, grid=16):
    """stress_scene(n): `ids` 2^k along x in frames 1 and 2, seen from beside the last of them.  With the ground (r = 1000) among them and
    k = 7 the view stays at home, where the ground is the moved sphere in view and the lattice the static ones, and in frame 2 the
    ground goes the other way"""
    def build():
        from toypathtracer_amd.scenes import stress_scene
        s, m = stress_scene(n, grid)
        c = centres_of(s, ids, 3)
        c[1:, :, 0] += f32(2.0 ** k)
        last = ids[-1]
        if 0 in ids and k < 10:
            c[2, ids.index(0), 0] -= f32(2.0 ** (k + 1))
            return _case(s, m, _stress_views(3), ids, c)
        v = [beside(c[j, -1], float(s["radius"][last])) for j in range(3)]
        if 0 in ids:
            v[0] = _stress_views(1)[0]
        return _case(s, m, v, ids, c)
    return build


def nine_moved(k):
    def build():
        s, m = _default()
        ids = list(REACH_IDS) + [8, 45, 2, 3, 5, 6]
        c = centres_of(s, ids, 3)
        c[1, :3, 0] += f32(2.0 ** k)
        c[2, 3:] += np.random.default_rng(9).uniform(-0.25, 0.25, (6, 3)).astype(f32)
        return _case(s, m, [HOME, _reach_view(s, c[1, :3]), HOME], ids, c)
    return build


for _k in (7, 20):
    _far = _k >= 10
    _add("ids", "ground_alone_2^%d" % _k, ground_alone(_k), no_static=(1,) if _far else ())
    _add("ids", "id_63_alone_of_64_2^%d" % _k, flat(64, [63], _k, 8), no_static=(1, 2) if _far else ())
    for _n in (65, 128, 255):
        _add("ids", "ids_0_63_of_%d_2^%d" % (_n, _k), flat(_n, [0, 63], _k), no_static=(1, 2) if _far else ())
    # the three calls that go frame by frame: one launch per frame
    _add("ids", "nine_moved_2^%d" % _k, nine_moved(_k), launches=3, no_static=(1,) if _far else ())
    _add("ids", "id_64_of_200_2^%d" % _k, flat(200, [3, 64], _k), launches=3, no_static=(1, 2) if _far else ())
    _add("ids", "two_of_256_2^%d" % _k, flat(256, [1, 200], _k), launches=3, no_static=(1, 2) if _far else ())


for _meta in META.values():
    _meta.setdefault("launches", 1)
FAMILIES = {family: tuple(b) for family, b in FAMILY_BUILDERS.items()}
CATALOGUE = {name: fn for b in FAMILY_BUILDERS.values() for name, fn in b.items()}
assert set(CATALOGUE) == set(META) and all(CATALOGUE.values())
FAMILY_OF = {name: META[name]["family"] for name in CATALOGUE}
FALLBACKS = tuple(n for n in CATALOGUE if n.startswith(("nine_moved", "id_64_of_200", "two_of_256")))
# one case per family for the runs with the scene forced into and out of LDS (every table_seam case is added to them)
ONE_PER_FAMILY = ("reach_2^20_mid", "tie_of_two_moved", "lights_far", "moved_negated_radius", "moved_8")
assert {FAMILY_OF[n] for n in ONE_PER_FAMILY} | {"table_seam"} == set(FAMILIES)

_built = {}


def case(name):
    """the case of this name, built once and shared read-only between the tests"""
    if name not in _built:
        c = CATALOGUE[name]()
        for a in c[:5]:
            a.setflags(write=False)
        _built[name] = c
    return _built[name]


# ---------------------------------------------------------------- the three time-driven calls
TIMES = (0.0, -0.0, float(f32(math.pi)), 1e-40, -2.5, 100.0, 1e6, 1e30, 3.4e38)


def animated_y1(t):
    """sphere 1's y at time t as tptUpdate moves it (Test.cpp:304-308), by the oracle"""
    from oracle_lib import Oracle
    s, _ = Oracle.get().default_scene()
    Oracle.get().animate(s, float(t))
    return f32(s["cy"][1])


def _timed(s, m, times, views=None, flags=FLAG_PROGRESSIVE | FLAG_ANIMATE, first=0):
    times = [float(t) for t in times]
    views = np.asarray([HOME] * len(times) if views is None else views, f32).reshape(len(times), 9)
    return s, m, times, views, flags, first


def timed_every_time():
    """the built-in scene at every time of TIMES, the repeated camera"""
    s, m = _default()
    return _timed(s, m, TIMES)


def timed_equal_times():
    s, m = _default()
    return _timed(s, m, (0.75, 0.75, 0.75))


def timed_lights():
    """sphere 1 emissive (it is the one that moves in y), sphere 8 not a light any more"""
    s, m = _default()
    m["emissive"][1] = (4.0, 3.0, 2.0)
    m["emissive"][8] = 0
    return _timed(s, m, (0.0, float(f32(math.pi)), -2.5))


def timed_glass_around_the_camera():
    """sphere 1 is glass and stands below the camera, 0.25 beside it: at t = 0 (y = 2) the camera is inside it, at the other times not"""
    s, m = _default()
    m["type"][1], m["ri"][1] = DIELECTRIC, f32(1.5)
    o = DEFAULT_CAMERA["look_from"]
    s["cx"][1], s["cz"][1] = f32(o[0] + 0.25), f32(o[2] - 0.125)
    return _timed(s, m, (-2.5, 0.0, float(f32(math.pi))))


def timed_tie_on_a_higher_static():
    """sphere 9 stands where sphere 1 is at rest, (2, 0, -1), with its radius: sphere 1 is there when cos t + 1 == 0, which the search
    finds at t = float32(pi); at the other times it is above"""
    s, m = _default()
    t = next(t for t in TIMES if animated_y1(t) == f32(0))
    s["cx"][9], s["cy"][9], s["cz"][9] = s["cx"][1], f32(0), s["cz"][1]
    v = beside((s["cx"][1], 0.0, s["cz"][1]), 0.5, side=(-0.6, 0.5, 1.0), fill=0.22)
    return _timed(s, m, (0.0, t, -2.5), [v, v, v])


def timed_tie_on_a_lower_static():
    """sphere 3 stands at (-1.5, 1.5, 0) with sphere 8's radius: sphere 8 (z = 0.3 sin t) is there at t = 0 and t = -0.0, and 0.18 in
    front of it at t = -2.5"""
    s, m = _default()
    s["cx"][3], s["cy"][3], s["cz"][3], s["radius"][3] = s["cx"][8], s["cy"][8], f32(0.0), s["radius"][8]
    s["invRadius"][3] = f32(1) / s["radius"][3]
    v = beside((s["cx"][8], s["cy"][8], 0.0), 0.3, side=(0.3, 0.4, 1.0), fill=0.22)
    return _timed(s, m, (-2.5, 0.0, -0.0), [v, v, v])


TIMED_SEAM_XZ = (223.6, 104.4)  # (x^2, z^2 and 2 x z all inside the table's range; r^2 - |c|^2 is what reaches the limit)


def timed_seam(x):
    """sphere 1 with r = 30 at (x, cos t + 1, 104.4): the table's term r^2 - |c|^2 + m_s passes the limit with y^2, so that the time
    decides on which side the scene lies (x is found by bisection at t = 0, tests/test_motion_kinds.py timed_seam_x)"""
    s, m = _default()
    s["cx"][1], s["cz"][1], s["radius"][1] = f32(x), f32(TIMED_SEAM_XZ[1]), f32(30)
    s["invRadius"][1] = f32(1) / f32(30)
    # from 90 units beside the sphere, half way between it and the ground: both in view
    o = np.array([float(f32(x)) + 38.0, 10.0, TIMED_SEAM_XZ[1] - 81.5])
    u1, u2 = np.array([float(f32(x)), 1.0, TIMED_SEAM_XZ[1]]) - o, np.array([0.0, -60.0, 0.0]) - o
    v = view(o, o + 50.0 * (u1 / np.linalg.norm(u1) + u2 / np.linalg.norm(u2)), vfov=80.0)
    return _timed(s, m, (float(f32(math.pi)), 0.0, float(f32(math.pi))), [v, v, v])


TIMED = {
    "timed_every_time": timed_every_time,
    "timed_equal_times": timed_equal_times,
    "timed_lights": timed_lights,
    "timed_glass_around_the_camera": timed_glass_around_the_camera,
    "timed_tie_on_a_higher_static": timed_tie_on_a_higher_static,
    "timed_tie_on_a_lower_static": timed_tie_on_a_lower_static,
}
_built_timed = {}


def timed(name):
    if name not in _built_timed:
        _built_timed[name] = TIMED[name]()
    return _built_timed[name]
