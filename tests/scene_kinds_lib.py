"""TEST INFRASTRUCTURE: scenes whose SPHERES, MATERIALS, SCALE and CAMERA are the subject, for tests/test_scene_kinds.py (the oracle and the
host restatement of the lane logic, on the CPU) and tests/test_gpu_scene_kinds.py (the trace kernels on the GPU).  Every builder is seeded
(most are deterministic edits of the built-in scene) and returns (spheres, materials, camera): the arrays in oracle_lib's record layouts,
`camera` None for the default camera or the keyword arguments of toypathtracer_amd.api.set_camera; oracle_camera() turns them into the
oracle's camera.  invRadius is always float32(1) / radius.  Nothing under toypathtracer_amd/ imports this module.

CATALOGUE maps a name (the test id) to its builder, FAMILIES a family to its names:

  materials     the built-in scene with roughness 0 / 1 / 4 / -0.5 on every metal, spheres 3..7 dielectric with ri 1, 1.0001, 0.5, 2.5,
                1e-3, 1e3, 0, -1.5, the albedo of spheres 1..45 at 0 / 1 / 2 / -0.5, and a `type` no class knows (3, -1, 0x7fffffff) on
                spheres 2, 3, 12, 20: the path ends there with the hit's emission (the Q_END class of the path-queue kernel);
  populations   every sphere of one class (Lambert, mirror, glass), the built-in scene inside a closed shell of each class (r = 12 around
                the origin: no path reaches the sky; the mirror also with r = -12, see closed_shell), a hollow glass sphere (a second
                sphere of radius -0.9 r inside sphere 7), a glass shell around the mirror sphere 3;
  degenerate    a zero radius, a negated radius on a glass, a metal and a Lambert sphere, ten coincident spheres, every sphere three
                times as big (they overlap), the camera at the centre of a glass, a Lambert and a metal sphere;
  placement     the scene and its camera scaled by 2^-12 ... 2^16, the ground at r = 2^7 ... 2^60, scene and camera moved out by
                100 ... 1e5 along (1, 0, -1) (|c|^2 = 2 d^2 passes 60000 at d = 173: 240 has no table either), a sphere of r = 30 around
                x = 244 ... 300 (the matrix-core filter's table ends where a sphere's |a_k| reaches 60000, here c_x^2), the camera
                244 ... 2000 units out with a narrow lens (a ray with |o|^2 >= 60000 keeps every sphere of the table);
  camera        vfov 179 and 0.01, aperture 5 and 0, a focus distance of 1e-3;
  grouped       toypathtracer_amd.scenes.stress_scene(1000, 20) with 200 negated radii, 50 coincident spheres, every non-light sphere
                glass, moved out by 240 and 1e4, zero radii in five groups (each dissolves its group into the big list) and 70 zero
                radii (the big list overflows: the scene is flat).

`kitchen_sink` (family "other") is the built-in scene with one unknown type, one negated glass radius, three coincident spheres, ri 0.5
on one dielectric and roughness 4 on one metal, for the other entry points.  It has no zero radius: its normal would not be finite.

KEPT OUT ON PURPOSE, because the bit pattern of a NaN is not part of the contract and byte equality is what these tests demand:
albedo 1e20 (the image is infinite), a scale of 2^18 and above (not finite), and a camera whose up vector is parallel to its view
direction (every pixel NaN).  A camera with another up vector than (0, 1, 0) is not in the catalogue either: tptSetCamera takes none."""
import math

import numpy as np

from oracle_lib import MATERIAL_DT, SPHERE_DT, Oracle

LAMBERT, METAL, DIELECTRIC = 0, 1, 2
DEFAULT_CAMERA = dict(look_from=(0.0, 2.0, 3.0), look_at=(0.0, 0.0, 0.0), vfov=60.0, aperture=0.02, focus_dist=3.0)
f32 = np.float32


def _finish(s, m, camera=None):
    with np.errstate(divide="ignore"):
        s["invRadius"] = f32(1.0) / s["radius"]
    return s, m, camera


def _default():
    s, m = Oracle.get().default_scene()
    assert len(s) == 46 and s["radius"][0] == 100 and m["type"][7] == DIELECTRIC and m["type"][5] == METAL and m["type"][2] == LAMBERT
    return s, m


def _stress():
    from toypathtracer_amd.scenes import STRESS_CAMERA, stress_scene
    s, m = stress_scene(1000, 20)
    return s, m, dict(STRESS_CAMERA)


def _append(s, m, sphere, material):
    s2, m2 = np.zeros(len(s) + 1, SPHERE_DT), np.zeros(len(m) + 1, MATERIAL_DT)
    s2[:-1], m2[:-1] = s, m
    s2[-1], m2[-1] = sphere, material
    return s2, m2


def oracle_camera(oracle, camera, w, h):
    """the keyword arguments of tpt.set_camera (None: the default camera) -> the oracle's camera at this size"""
    if camera is None:
        return oracle.default_camera(w, h)
    return oracle.camera(camera["look_from"], camera["look_at"], (0, 1, 0), camera["vfov"], w / h, camera["aperture"], camera["focus_dist"])


def _moved(camera, d):
    c = dict(camera)
    c["look_from"] = tuple(float(f32(a) + f32(b)) for a, b in zip(camera["look_from"], d))
    c["look_at"] = tuple(float(f32(a) + f32(b)) for a, b in zip(camera["look_at"], d))
    return c


def _translate(s, d):
    for k, v in zip(("cx", "cy", "cz"), d):
        s[k] = s[k] + f32(v)


# ---------------------------------------------------------------- materials on the built-in scene
def roughness(value):
    def build():
        s, m = _default()
        m["roughness"][m["type"] == METAL] = f32(value)
        return _finish(s, m)
    return build


def refraction_index(value):
    def build():
        s, m = _default()
        m["type"][3:8] = DIELECTRIC
        m["ri"][3:8] = f32(value)
        return _finish(s, m)
    return build


def albedo(value):
    def build():
        s, m = _default()
        m["albedo"][1:] = f32(value)
        return _finish(s, m)
    return build


UNKNOWN_TYPE_IDS = (2, 3, 12, 20)


def unknown_type(value):
    def build():
        s, m = _default()
        m["type"][list(UNKNOWN_TYPE_IDS)] = np.int32(value)
        return _finish(s, m)
    return build


# ---------------------------------------------------------------- class populations
def _of_class(m, kind, ids=slice(None)):
    m["type"][ids] = kind
    if kind == METAL:
        m["roughness"][ids] = 0
    if kind == DIELECTRIC:
        m["ri"][ids] = f32(1.5)


def one_class(kind):
    def build():
        s, m = _default()
        _of_class(m, kind)
        return _finish(s, m)
    return build


def closed_shell(kind, radius=12.0):
    """the built-in scene and its camera inside a sphere of r = 12 around the origin: no path reaches the sky.  A METAL shell of positive
    radius ends every path that reaches it: its normal points away from the scene, the reflected ray into the surface (Test.cpp:218-221).
    The mirror that does send its paths back has the radius negated: the normal (p - c) * invRadius then faces the scene."""
    def build():
        s, m = _default()
        s, m = _append(s, m, (0, 0, 0, radius, 0), (kind, (0.7, 0.7, 0.7), (0, 0, 0), 0, 1.5 if kind == DIELECTRIC else 0))
        return _finish(s, m)
    return build


def hollow_glass():
    s, m = _default()
    inner = s[7].copy()
    inner["radius"] = f32(-0.9) * s["radius"][7]
    s, m = _append(s, m, inner, m[7])
    return _finish(s, m)


def glass_shell_around_a_mirror():
    s, m = _default()
    shell = s[3].copy()
    shell["radius"] = f32(1.5) * s["radius"][3]
    s, m = _append(s, m, shell, m[7])
    return _finish(s, m)


# ---------------------------------------------------------------- degenerate spheres
def zero_radius():
    s, m = _default()
    s["radius"][5] = 0
    return _finish(s, m)


def negated_radius(i):
    def build():
        s, m = _default()
        s["radius"][i] = -s["radius"][i]
        return _finish(s, m)
    return build


COINCIDENT = (9, range(10, 20))  # spheres 10..19 are copies of sphere 9: the lowest index is the one hit


def coincident():
    s, m = _default()
    for k in ("cx", "cy", "cz", "radius"):
        s[k][10:20] = s[k][9]
    return _finish(s, m)


def overlapping():
    s, m = _default()
    s["radius"][1:] *= f32(3)
    return _finish(s, m)


def camera_inside(i):
    def build():
        s, m = _default()
        centre = tuple(float(s[k][i]) for k in ("cx", "cy", "cz"))
        return _finish(s, m, dict(look_from=centre, look_at=(0.0, 0.0, -1.5), vfov=90.0, aperture=0.0, focus_dist=3.0))
    return build


# ---------------------------------------------------------------- scale and placement
def scaled(log2):
    def build():
        k = f32(2.0 ** log2)
        s, m = _default()
        for name in ("cx", "cy", "cz", "radius"):
            s[name] *= k
        c = DEFAULT_CAMERA
        cam = dict(look_from=tuple(float(f32(v) * k) for v in c["look_from"]), look_at=c["look_at"], vfov=c["vfov"],
                   aperture=float(f32(c["aperture"]) * k), focus_dist=float(f32(c["focus_dist"]) * k))
        return _finish(s, m, cam)
    return build


def ground(log2):
    def build():
        s, m = _default()
        s["radius"][0] = f32(2.0 ** log2)
        s["cy"][0] = f32(-0.5) - s["radius"][0]
        return _finish(s, m)
    return build


def offset(d):
    def build():
        s, m = _default()
        _translate(s, (d, 0, -d))
        return _finish(s, m, _moved(DEFAULT_CAMERA, (d, 0, -d)))
    return build


def big_sphere_at(x):
    def build():
        s, m = _default()
        s["cx"][9], s["radius"][9] = f32(x), f32(30)
        return _finish(s, m)
    return build


def far_camera(distance):
    def build():
        s, m = _default()
        o = (0.0, distance / 2.0, float(distance))
        return _finish(s, m, dict(look_from=o, look_at=(0.0, 0.0, 0.0), vfov=2.0, aperture=0.02, focus_dist=float(f32(math.hypot(*o)))))
    return build


# ---------------------------------------------------------------- camera
def camera(**changes):
    def build():
        s, m = _default()
        return _finish(s, m, dict(DEFAULT_CAMERA, **changes))
    return build


# ---------------------------------------------------------------- grouped scenes
NEGATED_IN_GROUPS = range(100, 300)
COINCIDENT_IN_GROUPS = (499, range(500, 550))


def grouped_negated():
    s, m, cam = _stress()
    s["radius"][100:300] = -s["radius"][100:300]
    return _finish(s, m, cam)


def grouped_coincident():
    s, m, cam = _stress()
    for k in ("cx", "cy", "cz", "radius"):
        s[k][500:550] = s[k][499]
    return _finish(s, m, cam)


def grouped_glass():
    s, m, cam = _stress()
    dark = ~(m["emissive"] > 0).any(axis=1)
    _of_class(m, DIELECTRIC, dark)
    return _finish(s, m, cam)


def grouped_offset(d):
    def build():
        s, m, cam = _stress()
        _translate(s, (d, 0, -d))
        return _finish(s, m, _moved(cam, (d, 0, -d)))
    return build


ZEROS_IN_DISTINCT_GROUPS = (100, 300, 500, 700, 900)  # (tests/test_scene_kinds.py holds that these lie in five groups: emu_group_info)


def grouped_zero_radii():
    s, m, cam = _stress()
    s["radius"][list(ZEROS_IN_DISTINCT_GROUPS)] = 0
    return _finish(s, m, cam)


def flat_zero_radii():
    """70 zero radii all over the lattice: more dissolved groups than the big list of 64 holds, buildGroups leaves the scene flat"""
    s, m, cam = _stress()
    s["radius"][np.arange(70) * 14 + 10] = 0
    return _finish(s, m, cam)


# ---------------------------------------------------------------- the other entry points
KITCHEN_SINK = dict(unknown=2, negated=7, coincident=(9, (10, 11)), ri_half=3, rough=5)


def kitchen_sink():
    s, m = _default()
    k = KITCHEN_SINK
    m["type"][k["unknown"]] = 3
    s["radius"][k["negated"]] = -s["radius"][k["negated"]]
    first, copies = k["coincident"]
    for name in ("cx", "cy", "cz", "radius"):
        s[name][list(copies)] = s[name][first]
    m["type"][k["ri_half"]], m["ri"][k["ri_half"]] = DIELECTRIC, f32(0.5)
    assert m["type"][k["rough"]] == METAL
    m["roughness"][k["rough"]] = f32(4)
    return _finish(s, m)


def _named(prefix, fn, values, fmt="%g"):
    return {prefix + (fmt % v): fn(v) for v in values}


FAMILY_BUILDERS = {
    "materials": dict(
        **_named("roughness_", roughness, (0, 1, 4, -0.5)),
        **_named("ri_", refraction_index, (1, 1.0001, 0.5, 2.5, 1e-3, 1e3, 0, -1.5)),
        **_named("albedo_", albedo, (0, 1, 2, -0.5)),
        **_named("type_", unknown_type, (3, -1, 0x7fffffff), "%d")),
    "populations": {
        "all_lambert": one_class(LAMBERT), "all_mirror": one_class(METAL), "all_glass": one_class(DIELECTRIC),
        "shell_lambert": closed_shell(LAMBERT), "shell_mirror": closed_shell(METAL), "shell_glass": closed_shell(DIELECTRIC),
        "shell_mirror_inward": closed_shell(METAL, -12.0),
        "hollow_glass": hollow_glass, "glass_shell_around_a_mirror": glass_shell_around_a_mirror},
    "degenerate": dict(
        {"zero_radius": zero_radius},
        **{"negated_radius_%s" % n: negated_radius(i) for n, i in (("glass", 7), ("metal", 5), ("lambert", 2))},
        **{"coincident": coincident, "overlapping": overlapping},
        **{"camera_inside_%s" % n: camera_inside(i) for n, i in (("glass", 7), ("lambert", 2), ("metal", 5))}),
    "placement": dict(
        **_named("scale_2^", scaled, (-12, -8, 8, 16), "%d"),
        **_named("ground_2^", ground, (7, 10, 20, 30, 49, 60), "%d"),
        **_named("offset_", offset, (100, 240, 250, 1e5)),
        **_named("big_sphere_at_", big_sphere_at, (244, 244.9, 245, 300)),
        **_named("far_camera_", far_camera, (244, 246, 2000))),
    "camera": {"vfov_179": camera(vfov=179.0), "vfov_0.01": camera(vfov=0.01), "aperture_5": camera(aperture=5.0),
               "aperture_0": camera(aperture=0.0), "focus_0.001": camera(focus_dist=1e-3)},
    "grouped": {"grouped_negated": grouped_negated, "grouped_coincident": grouped_coincident, "grouped_glass": grouped_glass,
                "grouped_offset_240": grouped_offset(240), "grouped_offset_10000": grouped_offset(1e4),
                "grouped_zero_radii": grouped_zero_radii, "flat_zero_radii": flat_zero_radii},
    "other": {"kitchen_sink": kitchen_sink},
}
FAMILIES = {family: tuple(b) for family, b in FAMILY_BUILDERS.items()}
CATALOGUE = {name: fn for b in FAMILY_BUILDERS.values() for name, fn in b.items()}
assert len(CATALOGUE) == sum(len(b) for b in FAMILY_BUILDERS.values()), "two scenes share a name"
FAMILY_OF = {name: family for family, names in FAMILIES.items() for name in names}

# what each scene is, as tests/test_scene_kinds.py proves it from the CPU restatement (emu_group_info, emu_matrix_masks) and
# tests/test_gpu_scene_kinds.py holds tptGetSceneInfo against
NO_TABLE = ({"ground_2^%d" % k for k in (10, 20, 30, 49, 60)} | {"offset_240", "offset_250", "offset_100000", "big_sphere_at_245", "big_sphere_at_300",
            "scale_2^8", "scale_2^16"} | set(FAMILIES["grouped"]))
GROUPED = set(FAMILIES["grouped"]) - {"flat_zero_radii"}
CLOSED_SHELLS = ("shell_lambert", "shell_glass", "shell_mirror_inward")  # (the shells that return their paths to the scene)


def size_of(name):
    """(w, h, spp, frames) both test files render the scene at: the smallest at which both workgroups of a CU get work and the
    accumulation is exercised"""
    return (64, 36, 2, 2) if FAMILY_OF[name] == "grouped" else (96, 54, 2, 2)


_built = {}


def scene(name):
    """the scene of this name, built once and shared read-only between the tests"""
    if name not in _built:
        s, m, cam = CATALOGUE[name]()
        s.setflags(write=False)
        m.setflags(write=False)
        _built[name] = (s, m, cam)
    return _built[name]
