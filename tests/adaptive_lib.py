"""Test infrastructure for tptDrawDeviceAdaptive and tptAdaptiveSamplesDevice (test infrastructure only): ctypes bindings of
tests/adaptive_checker.c -- the CPU reference of the trace with a count per pixel and its sample-weighted blend, and the C statement of
the plan function --, compiled with oracle/Makefile's CFLAGS into a directory the caller gives, and plan_numpy, a vectorised float32
statement of the plan function: one array operation per step, in the order written, so every rounding is the C statement's."""
import ctypes as C
import os

import numpy as np

from aov_lib import build_checker
from moments_lib import GK
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE, FOLD_RECURSIVE, MATH_TPT, ROOT, SEED_PER_PIXEL, Params

ADAPTIVE_SOURCE = os.path.join(ROOT, "tests", "adaptive_checker.c")
LUM_FLOOR = np.float32(1e-2)  # include/tpt_hip.h: TPT_ADAPTIVE_LUM_FLOOR
MAX_COUNT = 2047


class AdaptiveChecker:
    def __init__(self, out_dir):
        self.lib = lib = build_checker(ADAPTIVE_SOURCE, out_dir, "libadaptive_checker.so")
        lib.adaptive_render.restype = C.c_int64
        lib.adaptive_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Params)] + [C.c_void_p] * 5
        lib.adaptive_plan.restype = C.c_int64
        lib.adaptive_plan.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]

    def render(self, spheres, mats, cam, w, h, counts, frame, flags=FLAG_PROGRESSIVE, backbuffer=None, moments=None, albedo=None,
               normal_depth=None, light_sampling=True, threads=0):
        """one adaptive frame blended IN PLACE into backbuffer / moments (zeroed planes when None); albedo / normal_depth: planes that
        keep their entries where a pixel's count is 0 (NaN-filled planes when None) -> (rays, backbuffer, moments, albedo, normal_depth)"""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        assert counts.shape == (h, w)
        if backbuffer is None:
            backbuffer = np.zeros((h, w, 4), np.float32)
        if moments is None:
            moments = np.zeros((h, w, 4), np.float32)
        if albedo is None:
            albedo = np.full((h, w, 4), np.nan, np.float32)
        if normal_depth is None:
            normal_depth = np.full((h, w, 4), np.nan, np.float32)
        for b in (backbuffer, moments, albedo, normal_depth):
            assert b.dtype == np.float32 and b.flags.c_contiguous and b.size == w * h * 4
        p = Params(w, h, 0, h, 1, frame, flags, SEED_PER_PIXEL, MATH_TPT, FOLD_RECURSIVE, threads, 0 if light_sampling else 1, 0, 0, 0.0)
        rays = int(self.lib.adaptive_render(spheres.ctypes.data, mats.ctypes.data, len(spheres), cam.ctypes.data, C.byref(p),
                                            backbuffer.ctypes.data, albedo.ctypes.data, normal_depth.ctypes.data, moments.ctypes.data,
                                            counts.ctypes.data))
        return rays, backbuffer, moments, albedo, normal_depth

    def frames(self, oracle, w, h, counts, frames, flags=FLAG_PROGRESSIVE, time=0.0, spheres=None, mats=None, cam=None, **kw):
        """frames 0..frames-1 with the same counts on a zeroed tile and moments plane, as MomentsChecker.frames -> (per-frame rays, tile,
        moments, planes of the LAST frame)"""
        if spheres is None:
            spheres, mats = oracle.default_scene()
        else:
            spheres = spheres.copy()
        if flags & FLAG_ANIMATE:
            oracle.animate(spheres, time)
        if cam is None:
            cam = oracle.default_camera(w, h)
        bb = np.zeros((h, w, 4), np.float32)
        mo = np.zeros((h, w, 4), np.float32)
        per = []
        alb = nd = None
        for f in range(frames):
            r, _, _, alb, nd = self.render(spheres, mats, cam, w, h, counts, f, flags, backbuffer=bb, moments=mo, **kw)
            per.append(r)
        return per, bb, mo, alb, nd

    def plan(self, moments, target_error, min_samples, max_samples, variance=True):
        """-> (counts [h, w] int32, variance plane [h, w, 4] or None, total); AssertionError for arguments the product refuses"""
        h, w = moments.shape[:2]
        assert moments.dtype == np.float32 and moments.flags.c_contiguous and moments.shape == (h, w, 4)
        counts = np.full((h, w), -7, np.int32)
        var = np.full((h, w, 4), np.nan, np.float32) if variance else None
        total = int(self.lib.adaptive_plan(w, h, moments.ctypes.data, target_error, min_samples, max_samples, counts.ctypes.data,
                                           var.ctypes.data if variance else None))
        assert total >= 0, "the checker refused the arguments"
        return counts, var, total


def plan_numpy(moments, target_error, min_samples, max_samples, details=False):
    """the plan function of include/tpt_hip.h on whole arrays -> (counts, variance plane, total); details: also a dict of the
    intermediates b*b, r, R, need and extra (every pixel's, counted or not) and of `counted` (valid and gw > 0)"""
    f32 = np.float32
    h, w = moments.shape[:2]
    with np.errstate(all="ignore"):
        m0, m1, S = moments[..., 0], moments[..., 1], moments[..., 3]
        valid = (S >= f32(1)) & (S <= np.finfo(np.float32).max)
        d = m1 - m0 * m0
        var = np.where(d > 0, d, f32(0)).astype(f32)
        b = m0 + LUM_FLOOR
        r = (var / (b * b)).astype(f32)

        def shifted(arr, oy, ox):
            ys, xs = np.arange(h) + oy, np.arange(w) + ox
            inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
            return arr[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)], inside

        gv = np.zeros((h, w), f32)
        gw = np.zeros((h, w), f32)
        for jy in range(3):
            for jx in range(3):
                rq, inside = shifted(r, jy - 1, jx - 1)
                vq, _ = shifted(valid, jy - 1, jx - 1)
                k = GK[jy] * GK[jx]
                take = inside & vq
                gv = np.where(take, gv + k * rq, gv)
                gw = np.where(take, gw + k, gw)
        te = f32(target_error)
        R = gv / gw
        need = R / (te * te)
        extra = (need - S).astype(f32)
        lo, hi = f32(min_samples), f32(max_samples)
        mid = np.ceil(np.where((extra > lo) & (extra < hi), extra, f32(0))).astype(np.int32)
        n = np.where(~(extra > lo), np.int32(min_samples), np.where(extra >= hi, np.int32(max_samples), mid)).astype(np.int32)
        n = np.where(valid & (gw > 0), n, np.int32(max(min_samples, 1))).astype(np.int32)
        out = np.zeros((h, w, 4), f32)
        out[..., 1] = np.where(valid, var / np.where(valid, S, f32(1)), f32(0))
        out[..., 3] = np.where(valid, S, f32(0))
        inner = dict(bb=(b * b).astype(f32), r=r, R=R, need=need, extra=extra, counted=valid & (gw > 0))
    if details:
        return n, out, int(n.astype(np.int64).sum()), inner
    return n, out, int(n.astype(np.int64).sum())


def clamp_counts(counts):
    return np.clip(counts, 0, MAX_COUNT).astype(np.int32)
