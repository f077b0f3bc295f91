"""Test infrastructure for tptDrawDeviceMoments and tptDenoiseDeviceVariance (test infrastructure only): ctypes bindings of
tests/moments_checker.c (the CPU reference of the trace side) and tests/variance_checker.c (the CPU statement of the filter), both
compiled with oracle/Makefile's CFLAGS into a directory the caller gives (a pytest temp directory), and variance_numpy, a vectorised
float32 statement of the filter -- one array operation per step, in the order written, so every rounding is the C statement's."""
import ctypes as C
import os

import numpy as np

from aov_lib import build_checker
from denoise_lib import DEMODULATE, HK, random_planes  # noqa: F401  (re-exported for the tests)
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE, FOLD_RECURSIVE, MATH_TPT, ROOT, SEED_PER_PIXEL, Params

MOMENTS_SOURCE = os.path.join(ROOT, "tests", "moments_checker.c")
VARIANCE_SOURCE = os.path.join(ROOT, "tests", "variance_checker.c")
GK = np.array([0.25, 0.5, 0.25], np.float32)
EPS = np.float32(1e-4)  # include/tpt_hip.h: TPT_DENOISE_VARIANCE_EPS


class MomentsChecker:
    def __init__(self, out_dir):
        self.lib = lib = build_checker(MOMENTS_SOURCE, out_dir, "libmoments_checker.so")
        lib.moments_render.restype = C.c_int64
        lib.moments_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Params)] + [C.c_void_p] * 4
        lib.tpto_render.restype = C.c_int64
        lib.tpto_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Params), C.c_void_p]

    def render(self, spheres, mats, cam, w, h, spp, frame, flags=FLAG_PROGRESSIVE, seed_mode=SEED_PER_PIXEL, backbuffer=None,
               moments=None, light_sampling=True, mitsuba_compare=False, threads=0):
        """-> (rays, backbuffer and moments blended like tpto_render's backbuffer, albedo [h, w, 4], normal_depth [h, w, 4])"""
        if backbuffer is None:
            backbuffer = np.zeros((h, w, 4), np.float32)
        if moments is None:
            moments = np.zeros((h, w, 4), np.float32)
        for b in (backbuffer, moments):
            assert b.dtype == np.float32 and b.flags.c_contiguous and b.size == w * h * 4
        alb = np.full((h, w, 4), np.nan, np.float32)
        nd = np.full((h, w, 4), np.nan, np.float32)
        p = Params(w, h, 0, h, spp, frame, flags, seed_mode, MATH_TPT, FOLD_RECURSIVE, threads, 0 if light_sampling else 1,
                   1 if mitsuba_compare else 0, 0, 0.0)
        rays = int(self.lib.moments_render(spheres.ctypes.data, mats.ctypes.data, len(spheres), cam.ctypes.data, C.byref(p),
                                           backbuffer.ctypes.data, alb.ctypes.data, nd.ctypes.data, moments.ctypes.data))
        return rays, backbuffer, moments, alb, nd

    def frames(self, oracle, w, h, spp, frames, flags=FLAG_PROGRESSIVE, time=0.0, spheres=None, mats=None, cam=None, **kw):
        """frames 0..frames-1 on a zeroed tile and moments plane (kFlagAnimate applied like UpdateTest does) -> (per-frame rays, tile,
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
            r, _, _, alb, nd = self.render(spheres, mats, cam, w, h, spp, f, flags, backbuffer=bb, moments=mo, **kw)
            per.append(r)
        return per, bb, mo, alb, nd


class VarianceChecker:
    def __init__(self, out_dir):
        self.lib = lib = build_checker(VARIANCE_SOURCE, out_dir, "libvariance_checker.so")
        lib.denoise_variance.restype = C.c_int
        lib.denoise_variance.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_float, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                                                                 C.c_float, C.c_uint]

    def run(self, colour, albedo, normal_depth, moments, samples, iterations=5, sigma_luminance=4.0, sigma_normal=0.0, sigma_depth=0.0,
            flags=0):
        """-> the filtered [h, w, 4] float32 image; AssertionError for arguments the product refuses"""
        h, w = colour.shape[:2]
        for a in (colour, albedo, normal_depth, moments):
            assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (h, w, 4))
        out = np.full((h, w, 4), np.nan, np.float32)
        rc = self.lib.denoise_variance(w, h, colour.ctypes.data, None if albedo is None else albedo.ctypes.data,
                                       None if normal_depth is None else normal_depth.ctypes.data,
                                       None if moments is None else moments.ctypes.data, samples, out.ctypes.data, iterations,
                                       sigma_luminance, sigma_normal, sigma_depth, flags)
        assert rc == 0, "the checker refused the arguments"
        return out


def inv2(s):
    s = np.float32(s)
    return np.float32(1.0) / (s * s) if s > 0 else np.float32(0.0)


def lum(r, g, b):
    f32 = np.float32
    return (f32(0.2126) * r + f32(0.7152) * g) + f32(0.0722) * b


def variance_numpy(colour, albedo, normal_depth, moments, samples, iterations=5, sigma_luminance=4.0, sigma_normal=0.0, sigma_depth=0.0,
                   flags=0):
    f32 = np.float32
    h, w = colour.shape[:2]
    demod = bool(flags & DEMODULATE)
    with np.errstate(all="ignore"):
        c = [colour[..., k].astype(f32) for k in range(3)]
        if demod:
            for k in range(3):
                a = albedo[..., k]
                c[k] = np.where(a > 0, c[k] / np.where(a > 0, a, f32(1)), c[k])
        d = moments[..., 1] - moments[..., 0] * moments[..., 0]
        v = np.where(d > 0, d, f32(0)) / f32(samples)
        if demod:
            la = lum(albedo[..., 0], albedo[..., 1], albedo[..., 2])
            la2 = la * la
            v = np.where(la2 > 0, v / np.where(la2 > 0, la2, f32(1)), v)
        v = v.astype(f32)
        sl2 = f32(sigma_luminance) * f32(sigma_luminance)
        inn, idd = inv2(sigma_normal), inv2(sigma_depth)
        nd = None if normal_depth is None else [normal_depth[..., k] for k in range(4)]

        def shifted(arr, oy, ox):
            ys, xs = np.arange(h) + oy, np.arange(w) + ox
            valid = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
            return arr[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)], valid

        for i in range(iterations):
            s = 1 << i
            gv = np.zeros((h, w), f32)
            gw = np.zeros((h, w), f32)
            for jy in range(3):
                for jx in range(3):
                    vq, valid = shifted(v, jy - 1, jx - 1)
                    k = GK[jy] * GK[jx]
                    gv = np.where(valid, gv + k * vq, gv)
                    gw = np.where(valid, gw + k, gw)
            il = f32(s) / (sl2 * (gv / gw) + EPS)
            lp = lum(c[0], c[1], c[2])
            sw = np.zeros((h, w), f32)
            sv = np.zeros((h, w), f32)
            sc = [np.zeros((h, w), f32) for _ in range(3)]
            for ky in range(5):
                for kx in range(5):
                    oy, ox = (ky - 2) * s, (kx - 2) * s
                    cq = []
                    for ck in c:
                        q, valid = shifted(ck, oy, ox)
                        cq.append(q)
                    vq, _ = shifted(v, oy, ox)
                    dl = lum(cq[0], cq[1], cq[2]) - lp
                    den = f32(1) + (dl * dl) * il
                    if nd is not None:
                        nq = [shifted(nk, oy, ox)[0] for nk in nd]
                        dn = [nq[k] - nd[k] for k in range(3)]
                        dnn = (dn[0] * dn[0] + dn[1] * dn[1]) + dn[2] * dn[2]
                        den = den * (f32(1) + dnn * inn)
                        dd = nq[3] - nd[3]
                        den = den * (f32(1) + (dd * dd) * idd)
                    wt = (HK[ky] * HK[kx]) / den
                    sw = np.where(valid, sw + wt, sw)
                    for k in range(3):
                        sc[k] = np.where(valid, sc[k] + wt * cq[k], sc[k])
                    sv = np.where(valid, sv + (wt * wt) * vq, sv)
            c = [sc[k] / sw for k in range(3)]
            v = sv / (sw * sw)
        out = np.empty((h, w, 4), f32)
        for k in range(3):
            if demod:
                a = albedo[..., k]
                out[..., k] = np.where(a > 0, c[k] * a, c[k])
            else:
                out[..., k] = c[k]
        out[..., 3] = colour[..., 3]
    return out


def random_moments(rng, colour, spread=1.0):
    """seeded moments consistent with a colour plane: mean luminance near the colour's, second moment above its square by a
    non-negative variance (some pixels exactly 0, a few below the square to exercise the clamp); .z 0, .w junk"""
    f32 = np.float32
    h, w = colour.shape[:2]
    m1 = lum(colour[..., 0], colour[..., 1], colour[..., 2]).astype(f32)
    var = (rng.random((h, w), dtype=f32) ** f32(2) * f32(spread)).astype(f32)
    var[rng.random((h, w)) < 0.1] = 0
    m2 = (m1 * m1 + var).astype(f32)
    low = rng.random((h, w)) < 0.05
    m2[low] = (m1[low] * m1[low] * f32(0.5)).astype(f32)
    mo = np.stack([m1, m2, np.zeros_like(m1), rng.random((h, w), dtype=f32)], axis=-1).astype(f32)
    return np.ascontiguousarray(mo)
