"""Test infrastructure for tptRectifyHistoryDevice (test infrastructure only): a ctypes binding of tests/rectify_checker.c (the CPU
statement of the pass, compiled with oracle/Makefile's CFLAGS into a directory the caller gives), rectify_numpy, a vectorised float32
statement -- one array operation per step, in the order written, so every rounding is the C statement's -- and the seeded planes the
tests feed both."""
import ctypes as C
import os

import numpy as np

from aov_lib import build_checker
from oracle_lib import ROOT

SOURCE = os.path.join(ROOT, "tests", "rectify_checker.c")
FLT_MAX = np.float32(3.40282347e38)
NAMES = ("colour", "moments", "variance")
SIZES = [(1, 1), (3, 2), (63, 5), (64, 4), (65, 9), (130, 67)]  # the tile (64 x 4) and halo seams in x and y, and the borders
f32 = np.float32


class RectifyChecker:
    def __init__(self, out_dir):
        self.lib = lib = build_checker(SOURCE, out_dir, "librectify_checker.so")
        lib.rectify_history.restype = C.c_int
        lib.rectify_history.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_float]

    def run(self, colour, moments, acc_colour, acc_moments, radius=1, gamma=1.0, rc=False, in_place=False):
        """-> (out_colour, out_moments, out_variance); AssertionError for arguments the product refuses (rc=True: the code).
        in_place: the colour and moments outputs are (copies of) the accumulated planes themselves"""
        h, w = colour.shape[:2]
        for a in (colour, moments, acc_colour, acc_moments):
            assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (h, w, 4)
        if in_place:
            acc_colour, acc_moments = acc_colour.copy(), acc_moments.copy()
            outs = [acc_colour, acc_moments, np.full((h, w, 4), np.nan, np.float32)]
        else:
            outs = [np.full((h, w, 4), np.nan, np.float32) for _ in range(3)]
        code = self.lib.rectify_history(w, h, colour.ctypes.data, moments.ctypes.data, acc_colour.ctypes.data, acc_moments.ctypes.data,
                                        *[o.ctypes.data for o in outs], radius, gamma)
        if rc:
            return code
        assert code == 0, "the checker refused the arguments"
        return tuple(outs)


def _finite(v):
    return np.abs(v) <= FLT_MAX


def _variance(mx, my, N):
    dd = my - mx * mx
    zero = np.zeros_like(N)
    return np.stack([zero, np.where(dd > 0, dd, f32(0)) / N, zero, N], axis=-1).astype(f32)


def rectify_numpy(colour, moments, acc_colour, acc_moments, radius=1, gamma=1.0, details=False):
    """-> (out_colour, out_moments, out_variance); details=True: also a dict of the per-pixel L, U (h, w, 3), a, the window variance and the masks"""
    h, w = colour.shape[:2]
    r, gamma = int(radius), f32(gamma)
    cur, acc, M = colour[..., :3], acc_colour[..., :3], acc_moments
    N = M[..., 3]
    with np.errstate(all="ignore"):
        inside = _finite(cur).all(axis=-1)
        through = ~(_finite(N) & (N > 1)) | ~inside | ~_finite(acc).all(axis=-1)
        # 1. the window: a pixel that does not count adds +0, which leaves a sum that started from +0 as it is
        v = np.zeros((h + 2 * r, w + 2 * r, 3), f32)
        v[r:r + h, r:r + w] = np.where(inside[..., None], cur, f32(0))
        cnt = np.zeros((h + 2 * r, w + 2 * r), f32)
        cnt[r:r + h, r:r + w] = inside
        nj, s, t = np.zeros((h + 2 * r, w), f32), np.zeros((h + 2 * r, w, 3), f32), np.zeros((h + 2 * r, w, 3), f32)
        for i in range(2 * r + 1):  # left to right
            q = v[:, i:i + w]
            nj = nj + cnt[:, i:i + w]
            s = s + q
            t = t + q * q
        n, S1, S2 = np.zeros((h, w), f32), np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32)
        for j in range(2 * r + 1):  # bottom to top
            n = n + nj[j:j + h]
            S1 = S1 + s[j:j + h]
            S2 = S2 + t[j:j + h]
        n = np.where(n > 0, n, f32(1))[..., None]  # (n == 0 only where the pixel passes through)
        mean = S1 / n
        var = S2 / n - mean * mean
        var = np.where(var < 0, f32(0), var)
        g = gamma * np.sqrt(var)
        lo, hi = mean - g, mean + g
        lo = np.where(lo < cur, lo, cur)
        hi = np.where(hi > cur, hi, cur)
        # 2. the clamp
        Ns = np.where(through, f32(2), N)
        lerp = ((Ns - f32(1)) / Ns)[..., None]
        one = f32(1) - lerp
        L, U = lo * lerp + cur * one, hi * lerp + cur * one
        out = np.where(acc < L, L, acc)
        out = np.where(out > U, U, out)
        # 3. the pull
        q = (acc - out) / (acc - cur)
        ac = np.where(~_finite(q), f32(1), np.where(q < 0, f32(0), np.where(q > 1, f32(1), q)))
        ac = np.where(out == acc, f32(0), ac).astype(f32)
        a = ac[..., 0]
        a = np.where(ac[..., 1] > a, ac[..., 1], a)
        a = np.where(ac[..., 2] > a, ac[..., 2], a)
        keep = through | (a == 0)
        # 4. the shortened history
        k = f32(1) - a
        N1 = f32(1) + (Ns - f32(1)) * k
        mx = M[..., 0] * k + moments[..., 0] * a
        my = M[..., 1] * k + moments[..., 1] * a
        zero = np.zeros((h, w), f32)
        oc = np.where(keep[..., None], acc_colour, np.concatenate([out, acc_colour[..., 3:]], axis=-1)).astype(f32)
        om = np.where(keep[..., None], M, np.stack([mx, my, zero, N1], axis=-1)).astype(f32)
        ov = np.where(keep[..., None], _variance(M[..., 0], M[..., 1], N), _variance(mx, my, N1)).astype(f32)
    outs = tuple(np.ascontiguousarray(x) for x in (oc, om, ov))
    if details:
        return outs, dict(L=L, U=U, a=np.where(through, f32(0), a), through=through, keep=keep, out=out, var=var)
    return outs


def luminance_moments(rng, colour, history):
    """a moments plane {l, l^2 + a little, 0, history} for a colour plane, as random_frame of temporal_lib makes them"""
    m1 = ((f32(0.2126) * colour[..., 0] + f32(0.7152) * colour[..., 1]) + f32(0.0722) * colour[..., 2]).astype(f32)
    m2 = (m1 * m1 + rng.random(m1.shape, dtype=f32) * f32(0.25)).astype(f32)
    return np.ascontiguousarray(np.stack([m1, m2, np.zeros_like(m1), np.broadcast_to(f32(history), m1.shape)], axis=-1).astype(f32))


def synthetic_case(w, h, seed=0):
    """-> (colour, moments, acc_colour, acc_moments) of a seeded case.  The left part of the image is noise of a wide range (loose
    bounds), the right part a smooth ramp with a little noise (tight bounds) and, where there is room, a block of one constant colour
    (a flat window: sd == 0).  The accumulated colour is the blend, by each pixel's own N, of this frame with an unrelated history, so
    some pixels lie inside their bounds and some are clipped below or above.  Planted: non-finite raw pixels (inside other pixels'
    windows), non-finite cur, acc and N, N == 1, N below 1, fractional N, an accumulated value equal to this frame's."""
    rng = np.random.default_rng([seed, w, h, 77])
    n = w * h
    colour = (rng.random((h, w, 4), dtype=f32) ** f32(3) * f32(4)).astype(f32)
    ramp = (f32(0.5) + np.arange(w, dtype=f32)[None, :, None] / f32(64) + np.arange(h, dtype=f32)[:, None, None] / f32(32)).astype(f32)
    smooth = (ramp + rng.random((h, w, 3), dtype=f32) * f32(0.05)).astype(f32)
    right = np.arange(w) >= w // 2
    colour[:, right, :3] = smooth[:, right]
    if w >= 24 and h >= 5:
        colour[h // 2 - 2:h // 2 + 3, w - 12:w - 3, :3] = (0.25, 0.5, 0.75)
    hist = (rng.random((h, w, 3), dtype=f32) * f32(3)).astype(f32)
    N = rng.choice(np.array([1, 1.5, 2, 2.25, 3, 4, 7.5, 8, 16], f32), size=(h, w)).astype(f32)
    lerp = ((N - f32(1)) / N)[..., None]
    acc = np.empty((h, w, 4), f32)
    acc[..., :3] = hist * lerp + colour[..., :3] * (f32(1) - lerp)
    near = rng.random((h, w)) < 0.4  # a history that agrees with this frame's neighbourhood: mostly inside the bounds
    acc[near, :3] = (colour[near, :3] + (rng.random((int(near.sum()), 3), dtype=f32) - f32(0.5)) * f32(0.02)).astype(f32)
    acc[..., 3] = rng.random((h, w), dtype=f32)
    moments = luminance_moments(rng, colour, 0.0)
    moments[..., 3] = rng.random((h, w), dtype=f32)
    acc_moments = luminance_moments(rng, acc, 1.0)
    acc_moments[..., 2] = 0
    acc_moments[..., 3] = N
    fc, fa, fm = colour.reshape(n, 4), acc.reshape(n, 4), acc_moments.reshape(n, 4)
    plant = lambda: rng.integers(0, n, max(1, n // 50))
    for value, plane, comp in ((np.nan, fc, 0), (np.inf, fc, 2), (-np.inf, fc, 1), (np.nan, fa, 1), (np.inf, fa, 0), (-np.inf, fa, 2),
                               (np.nan, fm, 3), (np.inf, fm, 3), (-np.inf, fm, 3), (0.5, fm, 3), (0.0, fm, 3), (-2.0, fm, 3)):
        plane[plant(), comp] = value
    same = plant()
    fa[same, :3] = fc[same, :3]
    return tuple(np.ascontiguousarray(a) for a in (colour, moments, acc, acc_moments))
