"""Test infrastructure for tptTraceRaysDevice (test infrastructure only): the ctypes binding of tests/rays_checker.c, the CPU reference of
the call, compiled with oracle/Makefile's CFLAGS into a directory the caller gives (a pytest temp directory); the two scenes the tests
trace; and the ray catalogue.  Nothing under toypathtracer_amd/ imports this module."""
import ctypes as C
import os

import numpy as np

from aov_lib import build_checker
from oracle_lib import FOLD_FORWARD, FOLD_RECURSIVE, MATH_TPT, ROOT, SEED_PER_PIXEL, Oracle, Params  # noqa: F401  (re-exported)

SOURCE = os.path.join(ROOT, "tests", "rays_checker.c")
GLASS, MIRROR, LIGHT = 7, 3, 45  # spheres of the built-in scene (Test.cpp:13-31): the glass sphere, a metal one, the big light


class RaysChecker:
    def __init__(self, out_dir):
        self.lib = lib = build_checker(SOURCE, out_dir, "librays_checker.so")
        lib.rays_trace.restype = C.c_int64
        lib.rays_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Params), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.camera_rays.restype = None
        lib.camera_rays.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.tpto_render.restype = C.c_int64
        lib.tpto_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Params), C.c_void_p]

    def camera_rays(self, cam, w, h, frame=0):
        """-> [h * w, 8] float32: the rays pixel (x, y)'s first sample of `frame` starts with, row 0 at the bottom, the RNG state left
        after the ray was made as the seed word"""
        out = np.full((h * w, 8), np.nan, np.float32)
        self.lib.camera_rays(cam.ctypes.data, w, h, frame, out.ctypes.data)
        return out

    def trace(self, spheres, mats, rays, radiance=True, hits=True, fold=FOLD_RECURSIVE, light_sampling=True, mitsuba_compare=False,
              threads=0):
        """-> (sum of k, radiance [n, 4] or None, hits [n, 8] or None): tptTraceRaysDevice on the host"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = len(rays)
        rad = np.full((n, 4), np.nan, np.float32) if radiance else None
        hit = np.full((n, 8), np.nan, np.float32) if hits else None
        p = Params(1, 1, 0, 1, 1, 0, 0, SEED_PER_PIXEL, MATH_TPT, fold, threads, 0 if light_sampling else 1, 1 if mitsuba_compare else 0,
                   0, 0.0)
        total = int(self.lib.rays_trace(spheres.ctypes.data, mats.ctypes.data, len(spheres), C.byref(p), n, rays.ctypes.data,
                                        None if rad is None else rad.ctypes.data, None if hit is None else hit.ctypes.data))
        return total, rad, hit

    def render(self, spheres, mats, cam, w, h, frame=0, fold=FOLD_RECURSIVE, light_sampling=True):
        """tpto_render at 1 spp with per-pixel seeds on a zeroed buffer, through this library's own copy of the oracle"""
        bb = np.zeros((h, w, 4), np.float32)
        p = Params(w, h, 0, h, 1, frame, 0, SEED_PER_PIXEL, MATH_TPT, fold, 0, 0 if light_sampling else 1, 0, 0, 0.0)
        rays = int(self.lib.tpto_render(spheres.ctypes.data, mats.ctypes.data, len(spheres), cam.ctypes.data, C.byref(p), bb.ctypes.data))
        return rays, bb


# ---------------------------------------------------------------- scenes
def default_scene():
    """the built-in 46 spheres: the lane-refill kernel stages them in LDS and filters them flat"""
    return Oracle.get().default_scene()


GROUPED_CAMERA = dict(look_from=(0.0, 6.0, 20.0), look_at=(0.0, 0.0, 0.0), vfov=60.0, aperture=0.02, focus_dist=20.0)


def grouped_scene():
    """toypathtracer_amd.scenes.stress_scene(320, 18): 320 spheres, which packScene groups (256 or more): read from global memory, the
    grouped traversal"""
    from toypathtracer_amd.scenes import stress_scene
    return stress_scene(320, 18)


SCENES = {"default": default_scene, "grouped": grouped_scene}


def scene_camera(name, w, h):
    o = Oracle.get()
    if name == "default":
        return o.default_camera(w, h)
    c = GROUPED_CAMERA
    return o.camera(c["look_from"], c["look_at"], (0.0, 1.0, 0.0), c["vfov"], w / h, c["aperture"], c["focus_dist"])


# ---------------------------------------------------------------- rays
def make_rays(origins, dirs, seeds):
    o, d = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
    r = np.zeros((len(o), 8), np.float32)
    r[:, 0:3], r[:, 4:7] = o, d
    r[:, 3] = np.asarray(seeds, np.uint32).view(np.float32)
    return r


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _seeds(n, salt):
    return ((np.arange(n, dtype=np.uint64) * 2654435761 + salt) % 0xFFFFFFFF + 1).astype(np.uint32)


def _sphere_dirs(n, rng):
    return _unit(rng.normal(size=(n, 3)))


def catalogue(checker, spheres, cam, seed=5):
    """name -> [n, 8] finite rays against `spheres` (any scene whose sphere 0 is the ground; the named spheres are taken from it):
      camera     camera_rays of a 40 x 25 frame
      inside     started at and around the centre of a glass sphere, in every direction
      surface    started ON a sphere's surface (the hit point of another ray's first hit, as the reference leaves it), outwards, inwards
                 and along the tangent plane: t = 0 is not a hit, kMinT decides
      sky        straight up and nearly so, from above everything: misses
      tangent    lines at distance r (1 - 1e-7 .. 1 + 1e-7) from a sphere's centre: the discriminant changes sign there
      far        from 1e3 .. 1e6 away towards the scene
      scaled     camera rays whose direction is NOT of unit length (x 0.5, x 2, x 37): the hit distances scale, the filters do not apply"""
    rng = np.random.default_rng(seed)
    s = spheres
    glass = GLASS if len(s) == 46 else int(np.argmax(s["radius"][5:]) + 5)
    c = np.array([s["cx"][glass], s["cy"][glass], s["cz"][glass]], np.float32)
    r = np.float32(s["radius"][glass])
    out = {}
    out["camera"] = checker.camera_rays(cam, 40, 25)
    # inside the sphere
    n = 96
    out["inside"] = make_rays(c + (rng.uniform(-0.5, 0.5, (n, 3)) * r).astype(np.float32), _sphere_dirs(n, rng), _seeds(n, 11))
    out["inside"][0, 0:3] = c  # (the centre itself)
    # on a surface: first hits of the camera rays
    _, _, hits = checker.trace(s, s_mats(checker, spheres), out["camera"][::7], radiance=False)
    on = hits[hits[:, 7].view(np.int32) >= 0][:64]
    pos, nrm = on[:, 0:3], on[:, 4:7]
    tang = _unit(np.cross(nrm, np.float32([0.3, 1.0, 0.2])) + 1e-3)
    k = len(on) // 3
    dirs = np.concatenate([_unit(nrm[:k]), _unit(-nrm[k:2 * k] + 0.2 * tang[k:2 * k]), tang[2 * k:]])
    out["surface"] = make_rays(pos, dirs, _seeds(len(on), 23))
    # up into the sky
    n = 40
    up = _unit(np.float32([0, 1, 0]) + rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32))
    up[0] = (0, 1, 0)
    out["sky"] = make_rays(rng.uniform(-3, 3, (n, 3)).astype(np.float32) + np.float32([0, 40, 0]), up, _seeds(n, 31))
    # tangent lines
    n = 90
    d = _sphere_dirs(n, rng)
    side = _unit(np.cross(d, _sphere_dirs(n, rng)))
    eps = np.repeat(np.float32([-1e-7, 0.0, 1e-7, -1e-5, 1e-5, -1e-3]), n // 6)
    p = c + side * (r * (np.float32(1) + eps))[:, None]
    out["tangent"] = make_rays(p - d * np.float32(4.0), d, _seeds(n, 41))
    # from far outside
    n = 60
    d = _sphere_dirs(n, rng)
    dist = np.float32(10.0) ** rng.uniform(3, 6, n).astype(np.float32)
    target = rng.uniform(-2, 2, (n, 3)).astype(np.float32) * np.float32([1, 0.25, 1])
    out["far"] = make_rays(target - d * dist[:, None], d, _seeds(n, 53))
    # directions that are not of unit length
    base = out["camera"][::5][:150].copy()
    base[:, 4:7] *= np.repeat(np.float32([0.5, 2.0, 37.0]), 50)[:len(base), None]
    out["scaled"] = base
    for name, v in out.items():
        assert v.dtype == np.float32 and v.shape[1] == 8 and np.isfinite(v[:, [0, 1, 2, 4, 5, 6]]).all(), name
    return out


_MATS = {}


def s_mats(checker, spheres):
    """(the materials do not matter for first hits: any array of the right length)"""
    from oracle_lib import MATERIAL_DT
    n = len(spheres)
    if n not in _MATS:
        _MATS[n] = np.zeros(n, MATERIAL_DT)
    return _MATS[n]


def all_rays(cat):
    """the catalogue as one buffer, and each entry's slice of it"""
    names = sorted(cat)
    at, where = 0, {}
    for n in names:
        where[n] = slice(at, at + len(cat[n]))
        at += len(cat[n])
    return np.ascontiguousarray(np.concatenate([cat[n] for n in names])), where
