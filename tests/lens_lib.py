"""Test infrastructure for tptDrawDeviceLens (test infrastructure only): the ctypes binding of tests/lens_checker.c, the CPU reference of
the call, compiled with oracle/Makefile's CFLAGS into a directory the caller gives (a pytest temp directory); the lenses and the scenes
the tests draw.  Nothing under toypathtracer_amd/ imports this module."""
import ctypes as C
import os

import numpy as np

from aov_lib import build_checker
from oracle_lib import FLAG_PROGRESSIVE, FOLD_FORWARD, FOLD_RECURSIVE, MATH_TPT, ROOT, SEED_PER_PIXEL, Oracle, Params  # noqa: F401

SOURCE = os.path.join(ROOT, "tests", "lens_checker.c")
EQUIRECT, FISHEYE, ORTHO = 1, 2, 3
KINDS = {"equirect": EQUIRECT, "fisheye": FISHEYE, "ortho": ORTHO}
TWO_PI, PI = float(np.float32(6.2831855)), float(np.float32(3.1415927))


class Lens(C.Structure):
    """include/tpt_hip.h: tptLens (a mirror of its own, so that the checker does not depend on the binding under test)"""
    _fields_ = [("kind", C.c_int), ("origin", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3),
                ("forward", C.c_float * 3), ("sx", C.c_float), ("sy", C.c_float), ("maxAngle", C.c_float)]


def make_lens(kind, origin=(0.0, 1.0, 0.5), forward=(0.0, -0.1, -1.0), up=(0.0, 1.0, 0.0), sx=None, sy=None, max_angle=None):
    """a Lens of this module with an orthonormal basis made in float64 (right = forward x up) and rounded to binary32; the spans default
    to the largest the call accepts for EQUIRECT, to a 180-degree circle for FISHEYE, to a 6 x 4 window for ORTHO"""
    f = np.asarray(forward, np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r = r / np.linalg.norm(r)
    u = np.cross(r, f)
    d = {EQUIRECT: (TWO_PI, PI, 0.0), FISHEYE: (2.0, 2.0, PI / 2), ORTHO: (6.0, 4.0, 0.0)}[kind]
    lens = Lens(kind=kind, sx=d[0] if sx is None else sx, sy=d[1] if sy is None else sy, maxAngle=d[2] if max_angle is None else max_angle)
    lens.origin[:] = [float(x) for x in np.asarray(origin, np.float32)]
    lens.right[:], lens.up[:], lens.forward[:] = ([float(x) for x in v.astype(np.float32)] for v in (r, u, f))
    return lens


def to_api(lens):
    """the binding's own Lens with the same bytes"""
    from toypathtracer_amd import api
    out = api.Lens()
    C.memmove(C.byref(out), C.byref(lens), C.sizeof(Lens))
    return out


class LensChecker:
    def __init__(self, out_dir):
        self.lib = lib = build_checker(SOURCE, out_dir, "liblens_checker.so")
        lib.lens_ray.restype = None
        lib.lens_ray.argtypes = [C.POINTER(Lens), C.c_float, C.c_float, C.c_void_p]
        lib.lens_render.restype = C.c_int64
        lib.lens_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Lens), C.POINTER(Params), C.c_void_p]
        lib.lens_sincos.restype = None
        lib.lens_sincos.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lens_rays.restype = None
        lib.lens_rays.argtypes = [C.POINTER(Lens), C.c_int, C.c_int, C.c_int, C.c_void_p]

    def sincos(self, x):
        """-> (tptm_sinf(x), tptm_cosf(x)) for a float32 array"""
        x = np.ascontiguousarray(x, np.float32)
        s, c = np.empty_like(x), np.empty_like(x)
        self.lib.lens_sincos(len(x), x.ctypes.data, s.ctypes.data, c.ctypes.data)
        return s, c

    def ray(self, lens, u, v):
        """-> [6] float32 {o, d}"""
        out = np.full(6, np.nan, np.float32)
        self.lib.lens_ray(C.byref(lens), float(np.float32(u)), float(np.float32(v)), out.ctypes.data)
        return out

    def ray_grid(self, lens, uv):
        """-> [n, 6] for uv [n, 2] float32"""
        return np.stack([self.ray(lens, u, v) for u, v in np.asarray(uv, np.float32)])

    def rays(self, lens, w, h, frame=0):
        """-> [h * w, 8] float32: tptTraceRaysDevice records of every pixel's first sample of `frame`"""
        out = np.full((h * w, 8), np.nan, np.float32)
        self.lib.lens_rays(C.byref(lens), w, h, frame, out.ctypes.data)
        return out

    def render(self, spheres, mats, lens, w, h, spp, frame=0, flags=0, backbuffer=None, fold=FOLD_RECURSIVE, light_sampling=True,
               threads=0):
        """-> (HitWorld calls, backbuffer [h, w, 4]): tptDrawDeviceLens on the host, blended into `backbuffer` (zeros if None)"""
        bb = np.zeros((h, w, 4), np.float32) if backbuffer is None else backbuffer
        assert bb.dtype == np.float32 and bb.flags.c_contiguous and bb.shape == (h, w, 4)
        p = Params(w, h, 0, h, spp, frame, flags, SEED_PER_PIXEL, MATH_TPT, fold, threads, 0 if light_sampling else 1, 0, 0, 0.0)
        rays = int(self.lib.lens_render(spheres.ctypes.data, mats.ctypes.data, len(spheres), C.byref(lens), C.byref(p), bb.ctypes.data))
        return rays, bb


def default_scene():
    """the built-in 46 spheres: the lane-refill kernel stages them in LDS and filters them flat"""
    return Oracle.get().default_scene()


def grouped_scene():
    """toypathtracer_amd.scenes.cloud_scene(320): spheres all around the lens, which packScene groups (256 or more)"""
    from toypathtracer_amd.scenes import cloud_scene
    return cloud_scene(320, extent=6.0, lights=6)


def noise_tile(w, h, seed=3):
    """a tile of NaN-free noise, alpha included"""
    return np.random.default_rng(seed).uniform(0.0, 2.0, (h, w, 4)).astype(np.float32)
