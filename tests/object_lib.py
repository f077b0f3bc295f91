"""Test infrastructure for tptObjectPlaneDevice and tptTemporalAccumulateObjectsDevice (test infrastructure only): a ctypes binding of
tests/object_checker.c (the CPU statements, compiled with oracle/Makefile's CFLAGS into a directory the caller gives), their numpy
twins -- one float32 array operation per step, in the order written, so every rounding is the C statement's -- and the cases the
tests feed both."""
import ctypes as C
import os

import numpy as np

from aov_lib import build_checker
from oracle_lib import FLAG_ANIMATE, ROOT, SPHERE_DT
from temporal_lib import FLT_MAX, KINDS, SNAP, _dot, _finite, camera_floats, look_at_camera, synthetic_case

SOURCE = os.path.join(ROOT, "tests", "object_checker.c")
f32 = np.float32
MIN_T, MAX_T = f32(0.001), f32(1.0e7)


def cameras_floats(cams):
    """a CAMERA_DT array (or N x 22 floats) -> contiguous float32[N, 22]"""
    a = np.ascontiguousarray(cams).view(np.float32).reshape(-1, 22)
    return a.copy()


class ObjectChecker:
    def __init__(self, out_dir):
        self.lib = lib = build_checker(SOURCE, out_dir, "libobject_checker.so")
        lib.object_plane.restype = C.c_int
        lib.object_plane.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_uint, C.c_void_p]
        lib.object_accumulate.restype = C.c_int
        lib.object_accumulate.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 14 + [C.c_float] * 4 + [C.c_void_p] * 3 + [C.c_int]

    def plane(self, spheres, cams, w, h, times=None, flags=0):
        """-> int32 [N, h, w]: the object planes of the N cameras (and times) over `spheres` (SPHERE_DT)"""
        c = cameras_floats(cams)
        n = c.shape[0]
        t = None if times is None else np.ascontiguousarray(times, np.float32)
        assert t is None or t.shape == (n,)
        s = np.ascontiguousarray(spheres)
        assert s.dtype == SPHERE_DT
        out = np.full((n, h, w), -2, np.int32)
        rc = self.lib.object_plane(n, None if t is None else t.ctypes.data, c.ctypes.data, w, h, s.ctypes.data, len(s), flags, out.ctypes.data)
        assert rc == 0, "the checker refused the arguments"
        return out

    def run(self, cam, cur, obj, prev=None, motion=None, max_history=4.0, depth_tolerance=0.1, normal_tolerance=0.25,
            coverage_tolerance=0.0):
        """cur: (colour, albedo, normal_depth, moments); obj: int32 [h, w]; prev: None or (camera, colour, albedo, normal_depth, moments,
        object); motion: None or float32 [n, 4] -> (out_colour, out_albedo, out_moments, out_variance)"""
        h, w = cur[0].shape[:2]
        planes = list(cur) + (list(prev[1:5]) if prev is not None else [])
        for a in planes:
            assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (h, w, 4)
        ids = [obj] + ([prev[5]] if prev is not None else [])
        for a in ids:
            assert a.dtype == np.int32 and a.flags.c_contiguous and a.shape == (h, w)
        c0 = camera_floats(cam)
        c1 = None if prev is None else camera_floats(prev[0])
        m = None if motion is None else np.ascontiguousarray(motion, np.float32)
        assert m is None or (m.ndim == 2 and m.shape[1] == 4)
        outs = [np.full((h, w, 4), np.nan, np.float32) for _ in range(4)]
        ptr = [a.ctypes.data for a in planes] + [None] * (8 - len(planes)) + [o.ctypes.data for o in outs]
        code = self.lib.object_accumulate(w, h, c0.ctypes.data, None if c1 is None else c1.ctypes.data, *ptr, max_history, depth_tolerance,
                                          normal_tolerance, coverage_tolerance, obj.ctypes.data,
                                          None if prev is None else prev[5].ctypes.data, None if m is None else m.ctypes.data,
                                          0 if m is None else m.shape[0])
        assert code == 0, "the checker refused the arguments"
        return tuple(outs)


def centre_rays(cam, w, h):
    """the rays through the pixel centres and the lens centre -> (origin float32[3], [dx, dy, dz] of float32 [h, w])"""
    c = camera_floats(cam)
    o, ll, H, V = (c[k:k + 3] for k in (0, 3, 6, 9))
    s = ((np.arange(w, dtype=f32) + f32(0.5)) / f32(w))[None, :]
    t = ((np.arange(h, dtype=f32) + f32(0.5)) / f32(h))[:, None]
    v = [((ll[k] + s * H[k]) + t * V[k]) - o[k] for k in range(3)]
    inv = f32(1) / np.sqrt(_dot(v, v))
    return o, [(v[k] * inv).astype(f32) for k in range(3)]


def object_plane_numpy(spheres, cam, w, h):
    """one camera over `spheres` as they stand -> int32 [h, w]"""
    o, d = centre_rays(cam, w, h)
    hit_t = np.full((h, w), MAX_T, f32)
    ids = np.full((h, w), -1, np.int32)
    with np.errstate(all="ignore"):
        for i in range(len(spheres)):
            s = spheres[i]
            co = [f32(s["cx"]) - o[0], f32(s["cy"]) - o[1], f32(s["cz"]) - o[2]]
            nb = (co[0] * d[0] + co[1] * d[1]) + co[2] * d[2]
            cc = ((co[0] * co[0] + co[1] * co[1]) + co[2] * co[2]) - f32(s["radius"]) * f32(s["radius"])
            discr = nb * nb - cc
            pos = discr > 0
            sq = np.sqrt(np.where(pos, discr, f32(0)))
            t = nb - sq
            t = np.where(t <= MIN_T, nb + sq, t)
            take = pos & (t > MIN_T) & (t < hit_t)
            ids = np.where(take, np.int32(i), ids)
            hit_t = np.where(take, t, hit_t).astype(f32)
    return np.ascontiguousarray(ids)


def object_numpy(cam, cur, obj, prev=None, motion=None, max_history=4.0, depth_tolerance=0.1, normal_tolerance=0.25,
                 coverage_tolerance=0.0):
    """temporal_lib.temporal_numpy with the three changes of tptTemporalAccumulateObjectsDevice"""
    colour, albedo, nd, moments = cur
    h, w = colour.shape[:2]
    c = camera_floats(cam)
    o = c[0:3]
    vals = [colour[..., 0], colour[..., 1], colour[..., 2], albedo[..., 0], albedo[..., 1], albedo[..., 2], albedo[..., 3],
            moments[..., 0], moments[..., 1]]
    N = np.ones((h, w), f32)
    with np.errstate(all="ignore"):
        if prev is not None:
            pc = camera_floats(prev[0])
            pcol, palb, pnd, pmo, pobj = prev[1:]
            po, pH, pV, pw = pc[0:3], pc[6:9], pc[9:12], pc[18:21]
            a = pc[3:6] - po
            f = -_dot(a, pw)
            hh, vv = _dot(pH, pH), _dot(pV, pV)
            cov = albedo[..., 3]
            _, d3 = centre_rays(cam, w, h)
            hit = cov > 0
            cs = np.where(hit, cov, f32(1))
            d = nd[..., 3] / cs
            n = [nd[..., k] / cs for k in range(3)]
            if motion is not None:
                m = np.ascontiguousarray(motion, f32)
                read = hit & (obj >= 0) & (obj < m.shape[0])
                entry = m[np.where(read, obj, 0)]
                cap = np.where(read, entry[..., 3], f32(0))
                rel = [np.where(read, ((o[k] + d3[k] * d) + entry[..., k]) - po[k], np.where(hit, (o[k] + d3[k] * d) - po[k], d3[k]))
                       for k in range(3)]
            else:
                cap = np.zeros((h, w), f32)
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
                    cnt &= pobj[gy, gx] == obj
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
                    for k in range(9):
                        hist[k] = np.where(cnt, hist[k] + b * tv[k], hist[k])
                    histN = np.where(cnt, histN + b * N1, histN)
            has = B > 0
            Bs = np.where(has, B, f32(1))
            Nh = histN / Bs + f32(1)
            Nh = np.where(Nh > f32(max_history), f32(max_history), Nh)
            Nh = np.where((cap >= 1) & (cap < Nh), cap, Nh)
            N = np.where(has, Nh, f32(1)).astype(f32)
            lerp = (N - f32(1)) / N
            vals = [np.where(has, (hist[k] / Bs) * lerp + vals[k] * (f32(1) - lerp), vals[k]) for k in range(9)]
        oc = np.stack([vals[0], vals[1], vals[2], colour[..., 3]], axis=-1).astype(f32)
        oa = np.stack(vals[3:7], axis=-1).astype(f32)
        zero = np.zeros((h, w), f32)
        om = np.stack([vals[7], vals[8], zero, N], axis=-1).astype(f32)
        dd = vals[8] - vals[7] * vals[7]
        ov = np.stack([zero, np.where(dd > 0, dd, f32(0)) / N, zero, N], axis=-1).astype(f32)
    return tuple(np.ascontiguousarray(x) for x in (oc, oa, om, ov))


N_IDS = 6  # ids of the synthetic object planes: -1 .. N_IDS - 1, of which the table covers 0 .. N_IDS - 3


def synthetic_objects(kind, w, h, seed=0):
    """temporal_lib.synthetic_case(kind) with object planes and a motion table -> (camera, cur, obj, prev or None (with its object
    plane), motion).  The ids come in 3 x 2 blocks of -1 .. N_IDS - 1; the previous plane is this one with one pixel in eight changed;
    the table has N_IDS - 2 entries (the two highest ids are out of its range), small displacements, and caps of 0, 1, 2, 2.5 and 0.5."""
    cam, cur, prev = synthetic_case(kind, w, h, seed)
    rng = np.random.default_rng([seed, w, h, KINDS.index(kind), 7])
    blocks = rng.integers(-1, N_IDS, ((h + 1) // 2, (w + 2) // 3)).astype(np.int32)
    obj = np.ascontiguousarray(np.repeat(np.repeat(blocks, 2, axis=0), 3, axis=1)[:h, :w])
    motion = np.zeros((N_IDS - 2, 4), f32)
    motion[:, :3] = (rng.standard_normal((N_IDS - 2, 3)) * 0.02).astype(f32)
    motion[0, :3] = 0
    motion[:, 3] = np.array([0, 1, 2, 2.5, 0.5][:N_IDS - 2], f32)
    if prev is None:
        return cam, cur, obj, None, motion
    pobj = obj.copy()
    change = rng.random((h, w)) < 0.125
    pobj[change] = rng.integers(-1, N_IDS, int(change.sum())).astype(np.int32)
    return cam, cur, obj, tuple(prev) + (np.ascontiguousarray(pobj),), motion


def sphere_frame(cam, centre, radius, w, h, rng, history=None):
    """one sphere seen through `cam`, rendered analytically through the centre rays: coverage 1 where the ray hits, sky elsewhere
    -> ((colour, albedo, normal_depth, moments), object plane: 0 on the sphere, -1 elsewhere)"""
    o, d = centre_rays(cam, w, h)
    ctr = np.asarray(centre, f32)
    co = [ctr[k] - o[k] for k in range(3)]
    nb = (co[0] * d[0] + co[1] * d[1]) + co[2] * d[2]
    cc = f32((co[0] * co[0] + co[1] * co[1]) + co[2] * co[2]) - f32(radius) * f32(radius)
    discr = nb * nb - cc
    hit = discr > 0
    t = (nb - np.sqrt(np.where(hit, discr, f32(0)))).astype(f32)
    hit &= t > MIN_T
    pos = [o[k] + d[k] * t for k in range(3)]
    n = [((pos[k] - ctr[k]) / f32(radius)).astype(f32) for k in range(3)]
    cov = hit.astype(f32)
    colour = (rng.random((h, w, 4), dtype=f32) + f32(0.25)).astype(f32)
    albedo = np.zeros((h, w, 4), f32)
    albedo[..., 0:3] = np.array([0.8, 0.4, 0.2], f32) * cov[..., None]
    albedo[..., 3] = cov
    nd = np.zeros((h, w, 4), f32)
    for k in range(3):
        nd[..., k] = np.where(hit, n[k], f32(0))
    nd[..., 3] = np.where(hit, t, f32(0))
    m1 = ((f32(0.2126) * colour[..., 0] + f32(0.7152) * colour[..., 1]) + f32(0.0722) * colour[..., 2]).astype(f32)
    last = np.zeros((h, w), f32) if history is None else np.full((h, w), history, f32)
    mo = np.stack([m1, m1 * m1 + f32(0.1), np.zeros_like(m1), last], axis=-1).astype(f32)
    obj = np.where(hit, np.int32(0), np.int32(-1)).astype(np.int32)
    return tuple(np.ascontiguousarray(a) for a in (colour, albedo, nd, mo)), np.ascontiguousarray(obj)


def moved_sphere_case(w, h, seed=0):
    """A sphere of radius 0.5 at C in this frame that stood at C + m in the previous one, m = 0.4 sideways; the camera stands still.
    -> (camera, cur, obj, prev (camera, four planes with N = 1, object plane), motion table of one entry {m, 0})"""
    rng = np.random.default_rng([seed, w, h, 99])
    cam = look_at_camera([0.0, 1.0, 4.0], [0.0, 0.0, 0.0], w, h, aperture=0.0)
    centre, move = np.array([-0.2, 0.0, 0.0], f32), np.array([0.4, 0.0, 0.0], f32)
    cur, obj = sphere_frame(cam, centre, 0.5, w, h, rng)
    prev, pobj = sphere_frame(cam, centre + move, 0.5, w, h, rng, history=1.0)
    motion = np.array([[move[0], move[1], move[2], 0.0]], f32)
    return cam, cur, obj, (cam,) + prev + (pobj,), motion


__all__ = ["FLAG_ANIMATE", "KINDS", "N_IDS", "ObjectChecker", "cameras_floats", "centre_rays", "moved_sphere_case",
           "object_numpy", "object_plane_numpy", "sphere_frame", "synthetic_objects"]
