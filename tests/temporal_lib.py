"""Test infrastructure for tptTemporalAccumulateDevice (test infrastructure only): a ctypes binding of tests/temporal_checker.c (the
CPU statement of the pass, compiled with oracle/Makefile's CFLAGS into a directory the caller gives), temporal_numpy, a vectorised
float32 statement -- one array operation per step, in the order written, so every rounding is the C statement's -- and the cameras and
planes the tests feed both."""
import ctypes as C
import os

import numpy as np

from aov_lib import build_checker
from oracle_lib import ROOT

SOURCE = os.path.join(ROOT, "tests", "temporal_checker.c")
SNAP = np.float32(1.0 / 128)  # include/tpt_hip.h: TPT_TEMPORAL_SNAP
FLT_MAX = np.float32(3.40282347e38)
PLANES = ("colour", "albedo", "normal_depth", "moments")
f32 = np.float32


def camera_floats(cam):
    """a CAMERA_DT record (or 22 floats) -> contiguous float32[22]"""
    a = np.ascontiguousarray(cam).view(np.float32).reshape(-1)
    assert a.size == 22, "a camera is 88 bytes"
    return a.copy()


class TemporalChecker:
    def __init__(self, out_dir):
        self.lib = lib = build_checker(SOURCE, out_dir, "libtemporal_checker.so")
        lib.temporal_accumulate.restype = C.c_int
        lib.temporal_accumulate.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 14 + [C.c_float] * 4

    def run(self, cam, cur, prev=None, max_history=4.0, depth_tolerance=0.1, normal_tolerance=0.25, coverage_tolerance=0.0, rc=False):
        """cur: (colour, albedo, normal_depth, moments); prev: None or (camera, colour, albedo, normal_depth, moments)
        -> (out_colour, out_albedo, out_moments, out_variance); AssertionError for arguments the product refuses (rc=True: the code)"""
        h, w = cur[0].shape[:2]
        planes = list(cur) + (list(prev[1:]) if prev is not None else [])
        for a in planes:
            assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (h, w, 4)
        c0 = camera_floats(cam)
        c1 = None if prev is None else camera_floats(prev[0])
        outs = [np.full((h, w, 4), np.nan, np.float32) for _ in range(4)]
        ptr = [a.ctypes.data for a in planes] + [None] * (8 - len(planes)) + [o.ctypes.data for o in outs]
        code = self.lib.temporal_accumulate(w, h, c0.ctypes.data, None if c1 is None else c1.ctypes.data, *ptr, max_history,
                                            depth_tolerance, normal_tolerance, coverage_tolerance)
        if rc:
            return code
        assert code == 0, "the checker refused the arguments"
        return tuple(outs)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _finite(v):
    return np.abs(v) <= FLT_MAX


def temporal_numpy(cam, cur, prev=None, max_history=4.0, depth_tolerance=0.1, normal_tolerance=0.25, coverage_tolerance=0.0):
    colour, albedo, nd, moments = cur
    h, w = colour.shape[:2]
    c = camera_floats(cam)
    o, ll, H, V = (c[k:k + 3] for k in (0, 3, 6, 9))
    vals = [colour[..., 0], colour[..., 1], colour[..., 2], albedo[..., 0], albedo[..., 1], albedo[..., 2], albedo[..., 3],
            moments[..., 0], moments[..., 1]]
    N = np.ones((h, w), f32)
    with np.errstate(all="ignore"):
        if prev is not None:
            pc = camera_floats(prev[0])
            pcol, palb, pnd, pmo = prev[1:]
            po, pH, pV, pw = pc[0:3], pc[6:9], pc[9:12], pc[18:21]
            a = pc[3:6] - po
            f = -_dot(a, pw)
            hh, vv = _dot(pH, pH), _dot(pV, pV)
            cov = albedo[..., 3]
            s = ((np.arange(w, dtype=f32) + f32(0.5)) / f32(w))[None, :]
            t = ((np.arange(h, dtype=f32) + f32(0.5)) / f32(h))[:, None]
            v = [((ll[k] + s * H[k]) + t * V[k]) - o[k] for k in range(3)]
            inv = f32(1) / np.sqrt(_dot(v, v))
            d3 = [v[k] * inv for k in range(3)]
            hit = cov > 0
            cs = np.where(hit, cov, f32(1))
            d = nd[..., 3] / cs
            n = [nd[..., k] / cs for k in range(3)]
            rel = [np.where(hit, (o[k] + d3[k] * d) - po[k], d3[k]) for k in range(3)]
            z = -_dot(rel, pw)
            kz = f / z
            q = [rel[k] * kz - a[k] for k in range(3)]
            px = _dot(q, pH) / hh * f32(w) - f32(0.5)
            py = _dot(q, pV) / vv * f32(h) - f32(0.5)
            ok = (z > 0) & _finite(px) & _finite(py)
            px, py = np.where(ok, px, f32(0)), np.where(ok, py, f32(0))

            def snapped(pv):
                i0 = np.floor(pv)
                fr = pv - i0
                lo, hi = fr < SNAP, fr > f32(1) - SNAP
                i0 = np.where(~lo & hi, i0 + f32(1), i0)
                fr = np.where(lo | hi, f32(0), fr)
                return i0, fr

            ix, fx = snapped(px)
            iy, fy = snapped(py)
            e = np.sqrt(_dot(rel, rel))
            B = np.zeros((h, w), f32)
            hist = [np.zeros((h, w), f32) for _ in range(9)]
            histN = np.zeros((h, w), f32)
            for j in range(2):
                for i in range(2):
                    b = (fx if i else f32(1) - fx) * (fy if j else f32(1) - fy)
                    qx, qy = ix + f32(i), iy + f32(j)
                    inside = (qx >= 0) & (qx <= f32(w - 1)) & (qy >= 0) & (qy <= f32(h - 1))
                    cnt = ok & (b > 0) & inside
                    gx = np.where(inside, qx, f32(0)).astype(np.int64)
                    gy = np.where(inside, qy, f32(0)).astype(np.int64)
                    tc, ta, tn, tm = pcol[gy, gx], palb[gy, gx], pnd[gy, gx], pmo[gy, gx]
                    N1 = tm[..., 3]
                    cnt &= (N1 >= 1) & (N1 <= FLT_MAX)
                    cnt &= _finite(tc[..., 0]) & _finite(tc[..., 1]) & _finite(tc[..., 2])
                    c1 = ta[..., 3]
                    cnt &= np.abs(cov - c1) <= f32(coverage_tolerance)
                    both = hit & (c1 > 0)
                    c1s = np.where(c1 > 0, c1, f32(1))
                    d1 = tn[..., 3] / c1s
                    depth_ok = np.abs(e - d1) <= f32(depth_tolerance) * e
                    dn = [n[k] - tn[..., k] / c1s for k in range(3)]
                    normal_ok = (dn[0] * dn[0] + dn[1] * dn[1]) + dn[2] * dn[2] <= f32(normal_tolerance)
                    cnt &= np.where(both, depth_ok & normal_ok, (cov == 0) & (c1 == 0))
                    B = np.where(cnt, B + b, B)
                    tv = [tc[..., 0], tc[..., 1], tc[..., 2], ta[..., 0], ta[..., 1], ta[..., 2], ta[..., 3], tm[..., 0], tm[..., 1]]
                    for m in range(9):
                        hist[m] = np.where(cnt, hist[m] + b * tv[m], hist[m])
                    histN = np.where(cnt, histN + b * N1, histN)
            has = B > 0
            Bs = np.where(has, B, f32(1))
            Nh = histN / Bs + f32(1)
            Nh = np.where(Nh > f32(max_history), f32(max_history), Nh)
            N = np.where(has, Nh, f32(1)).astype(f32)
            lerp = (N - f32(1)) / N
            vals = [np.where(has, (hist[m] / Bs) * lerp + vals[m] * (f32(1) - lerp), vals[m]) for m in range(9)]
        oc = np.stack([vals[0], vals[1], vals[2], colour[..., 3]], axis=-1).astype(f32)
        oa = np.stack(vals[3:7], axis=-1).astype(f32)
        zero = np.zeros((h, w), f32)
        om = np.stack([vals[7], vals[8], zero, N], axis=-1).astype(f32)
        dd = vals[8] - vals[7] * vals[7]
        ov = np.stack([zero, np.where(dd > 0, dd, f32(0)) / N, zero, N], axis=-1).astype(f32)
    return tuple(np.ascontiguousarray(x) for x in (oc, oa, om, ov))


def look_at_camera(look_from, look_at, w, h, vfov=60.0, aperture=0.02, focus=3.0):
    """a pinhole-frame camera record in the reference's layout (float32 throughout; not bit-identical to the reference's constructor,
    which the GPU tests take from tptGetSceneDesc) -> float32[22]"""
    lf, la = np.asarray(look_from, f32), np.asarray(look_at, f32)
    half_h = f32(np.tan(np.float64(vfov) * np.pi / 360.0))
    half_w = f32(w) / f32(h) * half_h
    ww = lf - la
    ww = (ww / f32(np.linalg.norm(ww))).astype(f32)
    uu = np.cross(np.array([0, 1, 0], f32), ww).astype(f32)
    uu = (uu / f32(np.linalg.norm(uu))).astype(f32)
    vv = np.cross(ww, uu).astype(f32)
    fo = f32(focus)
    ll = lf - (half_w * fo) * uu - (half_h * fo) * vv - fo * ww
    cam = np.concatenate([lf, ll, (f32(2) * half_w * fo) * uu, (f32(2) * half_h * fo) * vv, uu, vv, ww, [f32(aperture) / f32(2)]])
    return np.ascontiguousarray(cam.astype(f32))


def axis_camera(w, h, x0=0.0, pixel=1.0 / 64):
    """A camera at (x0, 0, 0) looking down -z whose frame, at distance 1, has pixels exactly `pixel` wide and high (powers of two and
    small integers only: every product of the projection is exact) -> float32[22]"""
    pw, ph = f32(pixel) * f32(w), f32(pixel) * f32(h)
    o = np.array([x0, 0, 0], f32)
    ll = np.array([f32(x0) - pw / f32(2), -ph / f32(2), -1], f32)
    cam = np.concatenate([o, ll, [pw, 0, 0], [0, ph, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0]])
    return np.ascontiguousarray(cam.astype(f32))


def random_frame(rng, h, w, history=None):
    """seeded planes of one frame in the shape tptDrawDeviceMoments writes them: colour, {albedo, coverage}, {normal, depth} x coverage,
    {l, l^2}.  Coverage is 0 (sky), 1 or a quarter step between.  With `history` (the N to plant) the moments' .w carries it."""
    colour = (rng.random((h, w, 4), dtype=f32) ** f32(3) * f32(4)).astype(f32)
    cov = rng.choice(np.array([0, 0.25, 0.5, 1, 1, 1, 1], f32), size=(h, w)).astype(f32)
    albedo = (rng.random((h, w, 4), dtype=f32) * cov[..., None]).astype(f32)
    albedo[..., 3] = cov
    n = rng.standard_normal((h, w, 3)).astype(f32)
    n /= np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), f32(1e-3)).astype(f32)
    depth = (f32(1) + rng.random((h, w), dtype=f32) * f32(8)).astype(f32)
    nd = (np.concatenate([n, depth[..., None]], axis=-1) * cov[..., None]).astype(f32)
    m1 = ((f32(0.2126) * colour[..., 0] + f32(0.7152) * colour[..., 1]) + f32(0.0722) * colour[..., 2]).astype(f32)
    m2 = (m1 * m1 + rng.random((h, w), dtype=f32)).astype(f32)
    low = rng.random((h, w)) < 0.05
    m2[low] = (m1[low] * m1[low] * f32(0.5)).astype(f32)
    last = rng.random((h, w), dtype=f32) if history is None else np.broadcast_to(f32(history), (h, w))
    mo = np.stack([m1, m2, np.zeros_like(m1), last], axis=-1).astype(f32)
    return tuple(np.ascontiguousarray(a) for a in (colour, albedo, nd, mo))


def plane_frame(rng, h, w, cam, depth_z=4.0, history=None):
    """a frame whose guides describe the plane z = -depth_z seen fully covered through the axis camera `cam`: normal (0, 0, 1), depth
    = the pinhole ray's parameter at the plane (made in float32 the way the pass makes its own ray) -> planes as random_frame"""
    colour, albedo, nd, mo = random_frame(rng, h, w, history)
    c = camera_floats(cam)
    o, ll, H, V = (c[k:k + 3] for k in (0, 3, 6, 9))
    s = ((np.arange(w, dtype=f32) + f32(0.5)) / f32(w))[None, :]
    t = ((np.arange(h, dtype=f32) + f32(0.5)) / f32(h))[:, None]
    v = [((ll[k] + s * H[k]) + t * V[k]) - o[k] + np.zeros((h, w), f32) for k in range(3)]
    inv = f32(1) / np.sqrt(_dot(v, v))
    dz = v[2] * inv
    albedo[..., 3] = 1
    nd[..., 0:2] = 0
    nd[..., 2] = 1
    nd[..., 3] = (f32(-depth_z) / dz).astype(f32)
    return colour, albedo, nd, mo


KINDS = ("first", "same", "moved", "behind", "outside")


def synthetic_case(kind, w, h, seed=0):
    """-> (camera, cur planes, prev or None) of a seeded case.  "first": no history.  "same": the previous camera is this one and the
    previous guides are this frame's, so every pixel's own tap agrees -- but for the NaN, infinities and history lengths below 1 planted
    in the history.  "moved": as "same" seen from a camera 5 cm to the side (fractional taps, points leaving the frame).  "behind" /
    "outside": a previous camera that looks away from / at a right angle to the scene."""
    rng = np.random.default_rng([seed, w, h, KINDS.index(kind)])
    cam = look_at_camera([0.0, 2.0, 3.0], [0.0, 0.0, 0.0], w, h)
    cur = random_frame(rng, h, w)
    if kind == "first":
        return cam, cur, None
    pcol, palb, _, pmo = random_frame(rng, h, w)
    palb[..., 3] = cur[1][..., 3]
    pnd = cur[2].copy()
    pmo[..., 3] = rng.integers(1, 6, (h, w)).astype(f32)
    n = w * h
    flat_c, flat_m = pcol.reshape(n, 4), pmo.reshape(n, 4)
    for value, plane, comp in ((np.nan, flat_c, 0), (np.inf, flat_c, 2), (-np.inf, flat_c, 1), (np.nan, flat_m, 3), (np.inf, flat_m, 3),
                               (0.5, flat_m, 3), (0.0, flat_m, 3), (-2.0, flat_m, 3)):
        plane[rng.integers(0, n, max(1, n // 40)), comp] = value
    pcam = {"same": cam, "moved": look_at_camera([0.05, 2.0, 3.0], [0.0, 0.0, 0.0], w, h),
            "behind": look_at_camera([0.0, 2.0, 3.0], [0.0, 4.0, 6.0], w, h),
            "outside": look_at_camera([0.0, 2.0, 3.0], [30.0, 2.0, 3.0], w, h)}[kind]
    return cam, cur, (pcam, pcol, palb, pnd, pmo)
