"""Test infrastructure for tptSpatialVarianceDevice (test infrastructure only): a ctypes binding of tests/spatial_variance_checker.c (the
CPU statement of the call, compiled with oracle/Makefile's CFLAGS into a directory the caller gives), spatial_variance_numpy, a
vectorised float32 statement -- one array operation per step and per tap, in the order written, so every rounding is the C
statement's -- and the seeded planes the tests feed both."""
import ctypes as C
import os

import numpy as np

from aov_lib import build_checker
from oracle_lib import ROOT

SOURCE = os.path.join(ROOT, "tests", "spatial_variance_checker.c")
FLT_MAX = np.float32(3.40282347e38)
SIZES = [(1, 1), (3, 2), (63, 5), (64, 4), (65, 9), (130, 67)]  # the tile (64 x 4) and halo seams in x and y, and the borders
RADII = (1, 2, 3)
KINDS = ("mixed", "all", "none", "checker", "corner")
f32 = np.float32


class SpatialVarianceChecker:
    def __init__(self, out_dir):
        self.lib = lib = build_checker(SOURCE, out_dir, "libspatial_variance_checker.so")
        lib.spatial_variance.restype = C.c_int
        lib.spatial_variance.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_float, C.c_float, C.c_int, C.c_float, C.c_float]

    def run(self, moments, normal_depth=None, samples_per_frame=1.0, min_samples=2.0, radius=1, sigma_normal=0.0, sigma_depth=0.0,
            rc=False):
        """moments, normal_depth: [h, w, 4] or [frames, h, w, 4] -> the variance plane(s) in the same shape; AssertionError for
        arguments the product refuses (rc=True: the code)"""
        shape = moments.shape
        frames, h, w = (1,) + shape[:2] if moments.ndim == 3 else shape[:3]
        for a in (moments, normal_depth):
            assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == shape and shape[-1] == 4)
        out = np.full(shape, np.nan, np.float32)
        code = self.lib.spatial_variance(w, h, frames, moments.ctypes.data, None if normal_depth is None else normal_depth.ctypes.data,
                                         out.ctypes.data, samples_per_frame, min_samples, radius, sigma_normal, sigma_depth)
        if rc:
            return code
        assert code == 0, "the checker refused the arguments"
        return out


def _finite(v):
    return np.abs(v) <= FLT_MAX


def inv2(s):
    s = f32(s)
    return f32(1.0) / (s * s) if s > 0 else f32(0.0)


def own_variance(moments):
    """step 0 -> (Vt [.., 4], N)"""
    with np.errstate(all="ignore"):
        N = moments[..., 3]
        N = np.where(_finite(N) & (N >= 1), N, f32(1)).astype(f32)
        dd = moments[..., 1] - moments[..., 0] * moments[..., 0]
        v = np.where(dd > 0, dd, f32(0)).astype(f32)
        zero = np.zeros_like(N)
        return np.stack([zero, v / N, zero, N], axis=-1).astype(f32), N


def estimated(moments, samples_per_frame=1.0, min_samples=2.0):
    """the pixels that do not pass through"""
    with np.errstate(all="ignore"):
        return (f32(samples_per_frame) * own_variance(moments)[1]).astype(f32) < f32(min_samples)


def spatial_variance_numpy(moments, normal_depth=None, samples_per_frame=1.0, min_samples=2.0, radius=1, sigma_normal=0.0,
                           sigma_depth=0.0, details=False):
    """the shapes of SpatialVarianceChecker.run; details: (the output, a dict of the intermediates est, any (a tap counted), W, S1, S2,
    e1 -- the last four of every pixel, estimated or not).  It takes any sigma and any counts, also those the call refuses"""
    if moments.ndim == 3:
        out = spatial_variance_numpy(moments[None], None if normal_depth is None else normal_depth[None], samples_per_frame, min_samples,
                                     radius, sigma_normal, sigma_depth, details)
        return (out[0][0], {k: v[0] for k, v in out[1].items()}) if details else out[0]
    F, h, w = moments.shape[:3]
    r = int(radius)
    with np.errstate(all="ignore"):
        in_, id_ = inv2(sigma_normal), inv2(sigma_depth)
        Vt, N = own_variance(moments)
        est = estimated(moments, samples_per_frame, min_samples)
        mx, my = moments[..., 0], moments[..., 1]
        counts = _finite(mx) & _finite(my)
        pad = lambda a, fill=0: np.pad(a, ((0, 0), (r, r), (r, r)) + ((0, 0),) * (a.ndim - 3), constant_values=fill)  # noqa: E731
        pmx, pmy, pc = pad(np.where(counts, mx, f32(0))), pad(np.where(counts, my, f32(0))), pad(counts, False)
        pnd = None if normal_depth is None else pad(normal_depth)
        W, S1, S2 = (np.zeros((F, h, w), f32) for _ in range(3))
        any_tap = np.zeros((F, h, w), bool)
        for j in range(2 * r + 1):  # bottom to top
            for i in range(2 * r + 1):  # left to right
                sl = (slice(None), slice(j, j + h), slice(i, i + w))
                ok = pc[sl]
                wt = np.ones((F, h, w), f32)
                if pnd is not None:
                    dn = pnd[sl] - normal_depth
                    den = f32(1) + ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]) * in_
                    den = den * (f32(1) + (dn[..., 3] * dn[..., 3]) * id_)
                    ok = ok & _finite(den)
                    wt = f32(1) / den
                # a tap that does not count adds +0, which leaves a sum that started from +0 as it is
                wt = np.where(ok, wt, f32(0)).astype(f32)
                W = W + wt
                S1 = S1 + wt * pmx[sl]
                S2 = S2 + wt * pmy[sl]
                any_tap |= ok
        Ws = np.where(any_tap, W, f32(1))
        e1, e2 = S1 / Ws, S2 / Ws
        ds = e2 - e1 * e1
        v = np.where(ds > 0, ds, f32(0)).astype(f32)
        zero = np.zeros_like(N)
        Ve = np.stack([zero, v / N, zero, N], axis=-1).astype(f32)
        out = np.ascontiguousarray(np.where((est & any_tap)[..., None], Ve, Vt).astype(f32))
        return (out, dict(est=est, any=any_tap, W=W, S1=S1, S2=S2, e1=e1)) if details else out


def synthetic_case(w, h, frames=1, kind="mixed", seed=0):
    """-> (moments, normal_depth), each [frames, h, w, 4], of a seeded case.  The moments are {l, l^2 + a little} of a noisy luminance
    on the left and a smooth one on the right, with, where there is room, a block of one value (a flat window: the estimate is
    exactly 0) and a block of moments near 1e20, whose e1*e1 overflows.  The guide is a wall and a floor with noise on the depth.
    .w, the history length N, by `kind`: "all" 1 everywhere (every pixel estimated at 1 spp and a threshold of 2), "none" 4
    everywhere, "checker" 1 and 4 alternating, "corner" 8 but for the one pixel at the tile corner (63, 3) (or the image's last),
    "mixed" a seeded choice.  Planted in every kind: NaN and infinite moments and guide pixels (inside other pixels' windows and at
    estimated pixels themselves); in "mixed" also N of 0, below 1, negative, fractional, NaN and infinite."""
    rng = np.random.default_rng([seed, w, h, frames, KINDS.index(kind), 91])
    n = frames * w * h
    l = (rng.random((frames, h, w), dtype=f32) ** f32(3) * f32(4)).astype(f32)
    ramp = (f32(0.5) + np.arange(w, dtype=f32)[None, None, :] / f32(64) + np.arange(h, dtype=f32)[None, :, None] / f32(32)).astype(f32)
    right = np.arange(w) >= w // 2
    l[:, :, right] = (ramp + rng.random((frames, h, w), dtype=f32) * f32(0.05)).astype(f32)[:, :, right]
    m2 = (l * l + rng.random((frames, h, w), dtype=f32) * f32(0.25) * (rng.random((frames, h, w)) < 0.5)).astype(f32)
    if w >= 24 and h >= 9:
        l[:, h // 2 - 4:h // 2 + 5, w - 12:w - 3] = 0.625
        m2[:, h // 2 - 4:h // 2 + 5, w - 12:w - 3] = 0.390625  # (0.625^2, exactly)
        l[:, 0:4, 4:10] = (f32(1e20) * (f32(1) + rng.random((frames, 4, 6), dtype=f32))).astype(f32)
        m2[:, 0:4, 4:10] = f32(3e38)
    if kind == "all":
        N = np.ones((frames, h, w), f32)
    elif kind == "none":
        N = np.full((frames, h, w), 4, f32)
    elif kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        N = np.broadcast_to(np.where((xx + yy) % 2 == 0, f32(1), f32(4)), (frames, h, w)).astype(f32)
    elif kind == "corner":
        N = np.full((frames, h, w), 8, f32)
        N[:, min(3, h - 1), min(63, w - 1)] = 1
    else:
        N = rng.choice(np.array([1, 1, 1, 1.5, 1.99, 2, 2.25, 3, 4, 16], f32), size=(frames, h, w)).astype(f32)
    moments = np.stack([l, m2, rng.random((frames, h, w), dtype=f32), N], axis=-1).astype(f32)
    nd = np.zeros((frames, h, w, 4), f32)
    wall = np.arange(w) < (2 * w) // 3
    nd[:, :, wall, :3] = (0.0, 0.0, 1.0)
    nd[:, :, ~wall, :3] = (0.0, 1.0, 0.0)
    nd[..., :3] += (rng.random((frames, h, w, 3), dtype=f32) - f32(0.5)) * f32(0.02)
    nd[..., 3] = f32(3) + np.arange(h, dtype=f32)[None, :, None] / f32(16) + rng.random((frames, h, w), dtype=f32) * f32(0.3)
    fm, fg = moments.reshape(n, 4), nd.reshape(n, 4)
    plant = lambda: rng.integers(0, n, max(1, n // 60))  # noqa: E731
    planted = [(np.nan, fm, 0), (np.inf, fm, 1), (-np.inf, fm, 0), (np.nan, fm, 1), (np.nan, fg, 0), (np.inf, fg, 3), (-np.inf, fg, 2),
               (np.nan, fg, 3)]
    if kind == "mixed":
        planted += [(np.nan, fm, 3), (np.inf, fm, 3), (-np.inf, fm, 3), (0.5, fm, 3), (0.0, fm, 3), (-2.0, fm, 3)]
    if n >= 6:
        for value, plane, comp in planted:
            plane[plant(), comp] = value
    return np.ascontiguousarray(moments), np.ascontiguousarray(nd)
