"""tptDenoiseDevice's a-trous filter twice over (test infrastructure only): tests/denoise_checker.c through ctypes, compiled with
oracle/Makefile's CFLAGS into a directory the caller gives (a pytest temp directory), and denoise_numpy, a vectorised float32 statement
of the same formula -- one array operation per step, in the order written, so every rounding is the checker's."""
import ctypes as C
import os

import numpy as np

from aov_lib import build_checker
from oracle_lib import ROOT

SOURCE = os.path.join(ROOT, "tests", "denoise_checker.c")
DEMODULATE = 1
HK = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], np.float32)


class DenoiseChecker:
    def __init__(self, out_dir):
        self.lib = lib = build_checker(SOURCE, out_dir, "libdenoise_checker.so")
        lib.denoise.restype = C.c_int
        lib.denoise.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                C.c_float, C.c_uint]

    def run(self, colour, albedo=None, normal_depth=None, iterations=5, sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0, flags=0):
        """-> the filtered [h, w, 4] float32 image; AssertionError for arguments the product refuses"""
        h, w = colour.shape[:2]
        for a in (colour, albedo, normal_depth):
            assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (h, w, 4))
        out = np.full((h, w, 4), np.nan, np.float32)
        rc = self.lib.denoise(w, h, colour.ctypes.data, None if albedo is None else albedo.ctypes.data,
                              None if normal_depth is None else normal_depth.ctypes.data, out.ctypes.data, iterations, sigma_colour,
                              sigma_normal, sigma_depth, flags)
        assert rc == 0, "the checker refused the arguments"
        return out


def inv2(s):
    s = np.float32(s)
    return np.float32(1.0) / (s * s) if s > 0 else np.float32(0.0)


def denoise_numpy(colour, albedo=None, normal_depth=None, iterations=5, sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0, flags=0):
    f32 = np.float32
    h, w = colour.shape[:2]
    demod = bool(flags & DEMODULATE)
    with np.errstate(all="ignore"):
        c = [colour[..., k].astype(f32) for k in range(3)]
        if demod:
            for k in range(3):
                a = albedo[..., k]
                c[k] = np.where(a > 0, c[k] / np.where(a > 0, a, f32(1)), c[k])
        ic0, inn, idd = inv2(sigma_colour), inv2(sigma_normal), inv2(sigma_depth)
        nd = None if normal_depth is None else [normal_depth[..., k] for k in range(4)]
        for i in range(iterations):
            s = 1 << i
            ic = ic0 * f32(4 ** i)
            sw = np.zeros((h, w), f32)
            sc = [np.zeros((h, w), f32) for _ in range(3)]
            for ky in range(5):
                ys = np.arange(h) + (ky - 2) * s
                vy = (ys >= 0) & (ys < h)
                ys = np.clip(ys, 0, h - 1)
                for kx in range(5):
                    xs = np.arange(w) + (kx - 2) * s
                    vx = (xs >= 0) & (xs < w)
                    xs = np.clip(xs, 0, w - 1)
                    valid = vy[:, None] & vx[None, :]
                    q = (ys[:, None], xs[None, :])
                    cq = [ck[q] for ck in c]
                    d = [cq[k] - c[k] for k in range(3)]
                    dc = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                    den = f32(1) + dc * ic
                    if nd is not None:
                        nq = [nk[q] for nk in nd]
                        dn = [nq[k] - nd[k] for k in range(3)]
                        dnn = (dn[0] * dn[0] + dn[1] * dn[1]) + dn[2] * dn[2]
                        den = den * (f32(1) + dnn * inn)
                        dd = nq[3] - nd[3]
                        den = den * (f32(1) + (dd * dd) * idd)
                    wt = (HK[ky] * HK[kx]) / den
                    sw = np.where(valid, sw + wt, sw)
                    for k in range(3):
                        sc[k] = np.where(valid, sc[k] + wt * cq[k], sc[k])
            c = [sc[k] / sw for k in range(3)]
        out = np.empty((h, w, 4), f32)
        for k in range(3):
            if demod:
                a = albedo[..., k]
                out[..., k] = np.where(a > 0, c[k] * a, c[k])
            else:
                out[..., k] = c[k]
        out[..., 3] = colour[..., 3]
    return out


def random_planes(rng, h, w):
    """seeded test planes: colour with a bright tail and some negatives-free zeros, albedo in [0, 1) with exact zeros in some
    channels, unit normals (some zero) and depths in [0, 20)"""
    f32 = np.float32
    colour = (rng.random((h, w, 4), dtype=f32) ** f32(3) * f32(4)).astype(f32)
    colour[rng.random((h, w)) < 0.05, :3] = 0
    albedo = rng.random((h, w, 4), dtype=f32)
    albedo[rng.random((h, w, 4)) < 0.1] = 0
    n = rng.standard_normal((h, w, 3)).astype(f32)
    n /= np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), f32(1e-3)).astype(f32)
    n[rng.random((h, w)) < 0.05] = 0
    nd = np.concatenate([n.astype(f32), (rng.random((h, w, 1), dtype=f32) * f32(20)).astype(f32)], axis=-1)
    return np.ascontiguousarray(colour), np.ascontiguousarray(albedo), np.ascontiguousarray(nd.astype(f32))
