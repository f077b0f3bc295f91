"""ctypes binding of tests/aov_checker.c, the CPU reference of tptDrawDeviceAov's first-hit planes (test infrastructure only).

The checker is compiled with oracle/Makefile's CFLAGS into a directory the caller gives (a pytest temp directory)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE, FOLD_RECURSIVE, MATH_TPT, ORACLE_DIR, ROOT, SEED_PER_PIXEL, Params

SOURCE = os.path.join(ROOT, "tests", "aov_checker.c")


def oracle_cflags():
    text = open(os.path.join(ORACLE_DIR, "Makefile")).read()
    m = re.search(r"^CFLAGS\s*=\s*(.*)$", text, flags=re.M)
    assert m, "oracle/Makefile: no CFLAGS line"
    return m.group(1).split()


def build_checker(source, out_dir, name):
    """`source` (a tests/*_checker.c) compiled with the oracle's flags as `out_dir`/`name`, loaded"""
    so = os.path.join(str(out_dir), name)
    cc = os.environ.get("CC", "gcc")
    subprocess.check_call([cc] + oracle_cflags() + ["-shared", "-o", so, source, "-lm"])
    return C.CDLL(so)


class AovChecker:
    def __init__(self, out_dir):
        self.lib = lib = build_checker(SOURCE, out_dir, "libaov_checker.so")
        lib.aov_render.restype = C.c_int64
        lib.aov_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.tpto_render.restype = C.c_int64
        lib.tpto_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Params), C.c_void_p]

    def render(self, spheres, mats, cam, w, h, spp, frame, flags=FLAG_PROGRESSIVE, seed_mode=SEED_PER_PIXEL, backbuffer=None,
               light_sampling=True, mitsuba_compare=False, threads=0):
        """-> (rays, backbuffer blended like tpto_render's, albedo [h, w, 4], normal_depth [h, w, 4])"""
        if backbuffer is None:
            backbuffer = np.zeros((h, w, 4), np.float32)
        assert backbuffer.dtype == np.float32 and backbuffer.flags.c_contiguous and backbuffer.size == w * h * 4
        alb = np.full((h, w, 4), np.nan, np.float32)
        nd = np.full((h, w, 4), np.nan, np.float32)
        p = Params(w, h, 0, h, spp, frame, flags, seed_mode, MATH_TPT, FOLD_RECURSIVE, threads, 0 if light_sampling else 1,
                   1 if mitsuba_compare else 0, 0, 0.0)
        rays = int(self.lib.aov_render(spheres.ctypes.data, mats.ctypes.data, len(spheres), cam.ctypes.data, C.byref(p),
                                       backbuffer.ctypes.data, alb.ctypes.data, nd.ctypes.data))
        return rays, backbuffer, alb, nd

    def frames(self, oracle, w, h, spp, frames, flags=FLAG_PROGRESSIVE, time=0.0, spheres=None, mats=None, cam=None, **kw):
        """frames 0..frames-1 on a zeroed tile (kFlagAnimate applied like UpdateTest does, common.oracle_frames) -> (per-frame rays,
        tile, planes of the LAST frame)"""
        if spheres is None:
            spheres, mats = oracle.default_scene()
        else:
            spheres = spheres.copy()
        if flags & FLAG_ANIMATE:
            oracle.animate(spheres, time)
        if cam is None:
            cam = oracle.default_camera(w, h)
        bb = np.zeros((h, w, 4), np.float32)
        per = []
        alb = nd = None
        for f in range(frames):
            r, _, alb, nd = self.render(spheres, mats, cam, w, h, spp, f, flags, backbuffer=bb, **kw)
            per.append(r)
        return per, bb, alb, nd
