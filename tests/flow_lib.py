"""Test infrastructure for tptMotionVectorsDevice (test infrastructure only): a ctypes binding of tests/flow_checker.c (the CPU
statement, compiled with oracle/Makefile's CFLAGS into a directory the caller gives), flow_numpy, its vectorised float32 twin -- one
array operation per step, in the order written, so every rounding is the C statement's -- and the synthetic clips the tests feed both
and the GPU."""
import ctypes as C
import os

import numpy as np

from aov_lib import build_checker
from object_lib import cameras_floats
from oracle_lib import ROOT
from temporal_lib import FLT_MAX, SNAP, _dot, _finite, axis_camera, camera_floats, look_at_camera, plane_frame, random_frame

SOURCE = os.path.join(ROOT, "tests", "flow_checker.c")
f32 = np.float32
N_IDS = 6  # ids of the synthetic object planes: -1 .. N_IDS - 1, of which the tables cover 0 .. N_IDS - 3
TOLERANCES = dict(depth_tolerance=0.1, normal_tolerance=0.25, coverage_tolerance=0.25)  # the synthetic clips' edges are planted for these


def _ptr(a):
    return None if a is None else a.ctypes.data


def _check(clip):
    """the arrays of a clip (see synthetic_clip) as contiguous arrays of the right types -> (n, h, w)"""
    n, h, w = clip["albedo"].shape[:3]
    for k in ("albedo", "nd"):
        assert clip[k].dtype == np.float32 and clip[k].flags.c_contiguous and clip[k].shape == (n, h, w, 4), k
    assert clip["cameras"].dtype == np.float32 and clip["cameras"].shape == (n, 22) and clip["cameras"].flags.c_contiguous
    if clip.get("objects") is not None:
        assert clip["objects"].dtype == np.int32 and clip["objects"].flags.c_contiguous and clip["objects"].shape == (n, h, w)
    if clip.get("motion") is not None:
        assert clip["motion"].dtype == np.float32 and clip["motion"].flags.c_contiguous and clip["motion"].shape[::2] == (n, 4)
    return n, h, w


class FlowChecker:
    def __init__(self, out_dir):
        self.lib = lib = build_checker(SOURCE, out_dir, "libflow_checker.so")
        lib.flow_motion.restype = C.c_int
        lib.flow_motion.argtypes = [C.c_int] * 3 + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4 + [C.c_float] * 3 + [C.c_void_p]

    def run(self, clip, objects=True, table=True, prev=True, depth_tolerance=0.1, normal_tolerance=0.25, coverage_tolerance=0.0, rc=False):
        """clip: dict(cameras [n, 22], albedo, nd [n, h, w, 4], objects [n, h, w] int32, motion [n, k, 4], prev = (camera, albedo, nd,
        object)); objects / table / prev: whether the call is given them -> float32 [n, h, w, 4]"""
        n, h, w = _check(clip)
        obj = clip["objects"] if objects else None
        mo = clip["motion"] if objects and table else None
        pv = clip["prev"] if prev else None
        pcam = None if pv is None else camera_floats(pv[0])
        out = np.full((n, h, w, 4), np.nan, np.float32)
        code = self.lib.flow_motion(w, h, n, _ptr(clip["cameras"]), _ptr(clip["albedo"]), _ptr(clip["nd"]), _ptr(obj), _ptr(mo),
                                    0 if mo is None else mo.shape[1], _ptr(pcam), None if pv is None else _ptr(pv[1]),
                                    None if pv is None else _ptr(pv[2]), None if pv is None or obj is None else _ptr(pv[3]),
                                    depth_tolerance, normal_tolerance, coverage_tolerance, _ptr(out))
        if rc:
            return code
        assert code == 0, "the checker refused the arguments"
        return out


def flow_frame_numpy(cam, albedo, nd, obj, motion, pcam, palb, pnd, pobj, depth_tolerance, normal_tolerance, coverage_tolerance):
    """one frame against its predecessor (obj / pobj None: the plain form; motion None: no table) -> float32 [h, w, 4]"""
    h, w = albedo.shape[:2]
    c, pc = camera_floats(cam), camera_floats(pcam)
    o, ll, H, V = (c[k:k + 3] for k in (0, 3, 6, 9))
    po, pH, pV, pw = pc[0:3], pc[6:9], pc[9:12], pc[18:21]
    with np.errstate(all="ignore"):
        a = pc[3:6] - po
        f = -_dot(a, pw)
        hh, vv = _dot(pH, pH), _dot(pV, pV)
        xs, ys = np.arange(w, dtype=f32)[None, :], np.arange(h, dtype=f32)[:, None]
        s, t = (xs + f32(0.5)) / f32(w), (ys + f32(0.5)) / f32(h)
        v = [((ll[k] + s * H[k]) + t * V[k]) - o[k] for k in range(3)]
        inv = f32(1) / np.sqrt(_dot(v, v))
        d3 = [(v[k] * inv).astype(f32) for k in range(3)]
        cov = albedo[..., 3]
        hit = cov > 0
        cs = np.where(hit, cov, f32(1))
        d = nd[..., 3] / cs
        n = [nd[..., k] / cs for k in range(3)]
        at = [o[k] + d3[k] * d for k in range(3)]
        if obj is not None and motion is not None:
            read = hit & (obj >= 0) & (obj < motion.shape[0])
            entry = motion[np.where(read, obj, 0)]
            at = [np.where(read, at[k] + entry[..., k], at[k]) for k in range(3)]
        rel = [np.where(hit, at[k] - po[k], d3[k]).astype(f32) for k in range(3)]
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
            return i0.astype(f32), fr.astype(f32)

        fx0, fx = snapped(px)
        fy0, fy = snapped(py)
        e = np.sqrt(_dot(rel, rel))
        near = (px >= -1) & (px < f32(w)) & (py >= -1) & (py < f32(h))
        W = np.zeros((h, w), f32)
        for j in range(2):
            for i in range(2):
                b = (fx if i else f32(1) - fx) * (fy if j else f32(1) - fy)
                qx, qy = fx0 + f32(i), fy0 + f32(j)
                inside = (qx >= 0) & (qx <= f32(w - 1)) & (qy >= 0) & (qy <= f32(h - 1))
                cnt = ok & near & (b > 0) & inside
                gx = np.where(cnt, qx, f32(0)).astype(np.int64)
                gy = np.where(cnt, qy, f32(0)).astype(np.int64)
                ta, tn = palb[gy, gx], pnd[gy, gx]
                if obj is not None:
                    cnt &= pobj[gy, gx] == obj
                c1 = ta[..., 3]
                cnt &= np.abs(cov - c1) <= f32(coverage_tolerance)
                both = hit & (c1 > 0)
                c1s = np.where(c1 > 0, c1, f32(1))
                d1 = tn[..., 3] / c1s
                depth_ok = np.abs(e - d1) <= f32(depth_tolerance) * e
                dn = [n[k] - tn[..., k] / c1s for k in range(3)]
                normal_ok = (dn[0] * dn[0] + dn[1] * dn[1]) + dn[2] * dn[2] <= f32(normal_tolerance)
                cnt &= np.where(both, depth_ok & normal_ok, (cov == 0) & (c1 == 0))
                W = np.where(cnt, W + b, W).astype(f32)
        zero = np.zeros((h, w), f32)
        out = np.stack([np.where(ok, (fx0 + fx) - xs, zero), np.where(ok, (fy0 + fy) - ys, zero), np.where(ok, e, zero),
                        np.where(ok, W, zero)], axis=-1).astype(f32)
    return np.ascontiguousarray(out)


def flow_numpy(clip, objects=True, table=True, prev=True, depth_tolerance=0.1, normal_tolerance=0.25, coverage_tolerance=0.0):
    """FlowChecker.run's arguments -> float32 [n, h, w, 4]"""
    n, h, w = _check(clip)
    out = np.zeros((n, h, w, 4), f32)
    for j in range(n):
        if j == 0 and not prev:
            continue
        pcam, palb, pnd, pobj = (clip["cameras"][j - 1], clip["albedo"][j - 1], clip["nd"][j - 1], clip["objects"][j - 1]) if j else clip["prev"]
        out[j] = flow_frame_numpy(clip["cameras"][j], clip["albedo"][j], clip["nd"][j], clip["objects"][j] if objects else None,
                                  clip["motion"][j] if objects and table else None, pcam, palb, pnd, pobj if objects else None,
                                  depth_tolerance, normal_tolerance, coverage_tolerance)
    return out


KINDS = ("same", "moved", "pixel", "away")


def _cameras(kind, w, h):
    """-> (prev camera, [camera 0, camera 1, camera 2]): three frames whose predecessors differ, so that a frame read with another
    frame's constants changes bytes"""
    if kind == "same":  # nothing moves between frames 0, 1 and 2; the clip's predecessor stood elsewhere
        cam = look_at_camera([0.0, 2.0, 3.0], [0.0, 0.0, 0.0], w, h)
        return look_at_camera([0.03, 2.0, 3.0], [0.0, 0.0, 0.0], w, h), [cam, cam, cam]
    if kind == "moved":  # fractional taps, points leaving the frame
        return (look_at_camera([-0.05, 2.0, 3.0], [0.0, 0.0, 0.0], w, h),
                [look_at_camera([0.05 * j, 2.0 + 0.02 * j, 3.0], [0.0, 0.0, 0.0], w, h) for j in range(3)])
    if kind == "pixel":  # the axis camera over the plane z = -1, whose pixels are 1/64 wide there: shifts of 2 pixels, of 1/256 of a
        # pixel (below the snap) and of 1 - 1/256 + 1/4 of a pixel (no snap)
        x = [0.0, 2.0 / 64, 2.0 / 64 + 1.0 / (64 * 256), 2.0 / 64 + 1.0 / (64 * 256) + (1.25 - 1.0 / 256) / 64]
        return axis_camera(w, h, x[0]), [axis_camera(w, h, x[1 + j]) for j in range(3)]
    if kind == "away":  # frame 0 looks the opposite way of its predecessor (z <= 0 for every point), frame 1 at a right angle to frame 0
        # (most points leave the previous image)
        cam = look_at_camera([0.0, 2.0, 3.0], [0.0, 0.0, 0.0], w, h)
        return (look_at_camera([0.0, 2.0, 3.0], [-30.0, 2.0, 3.0], w, h),
                [look_at_camera([0.0, 2.0, 3.0], [30.0, 2.0, 3.0], w, h), cam, look_at_camera([0.0, 2.0, 3.2], [0.0, 0.0, 0.0], w, h)])
    raise ValueError(kind)


def synthetic_clip(kind, w, h, seed=0):
    """A seeded clip of three frames and its predecessor -> dict(cameras, albedo, nd, objects, motion, prev).  Every frame starts from
    one base frame (coverage in {0, 0.25, 0.5, 1}, seeded normals and depths; for "pixel" the plane z = -1 fully covered), so that taps
    agree wherever nothing is planted, and then differs from it: one pixel in eight is another frame's, and steps at the edges of
    TOLERANCES are planted -- depths scaled by 1 +- depthTolerance and a little more, normals turned to about normalTolerance, coverage a
    quarter or a half off -- beside NaN and infinite entries.  The ids come in 3 x 2 blocks of -1 .. N_IDS - 1, one pixel in eight
    changed per frame; the tables have N_IDS - 2 entries (the two highest ids are out of range) with small displacements, entry 0 zero,
    and a .w that must be ignored (NaN in places)."""
    rng = np.random.default_rng([seed, w, h, KINDS.index(kind), 11])
    pcam, cams = _cameras(kind, w, h)

    def base_frame(cam):
        planes = plane_frame(rng, h, w, cam, depth_z=1.0) if kind == "pixel" else random_frame(rng, h, w)
        return planes[1].copy(), planes[2].copy()

    balb, bnd = base_frame(cams[0])
    blocks = rng.integers(-1, N_IDS, ((h + 1) // 2, (w + 2) // 3)).astype(np.int32)
    bobj = np.ascontiguousarray(np.repeat(np.repeat(blocks, 2, axis=0), 3, axis=1)[:h, :w])
    n = w * h

    def frame(cam):
        alb, nd = (balb.copy(), bnd.copy()) if kind != "pixel" else base_frame(cam)
        obj = bobj.copy()
        oalb, ond = base_frame(cam)
        other = rng.random((h, w)) < 0.125
        alb[other], nd[other] = oalb[other], ond[other]
        change = rng.random((h, w)) < 0.125
        obj[change] = rng.integers(-1, N_IDS, int(change.sum())).astype(np.int32)
        fa, fn = alb.reshape(n, 4), nd.reshape(n, 4)
        pick = lambda: rng.integers(0, n, max(1, n // 24))
        for scale in (1.1, 0.9, 1.1001, 0.8999, 1.25):  # depth steps about depthTolerance = 0.1
            fn[pick(), 3] *= f32(scale)
        k = pick()  # normals turned so that |n - n'|^2 is about normalTolerance = 0.25: add 0.5 x coverage along x
        fn[k, 0] += f32(0.5) * fa[k, 3]
        k = pick()
        fn[k, 0] += f32(0.51) * fa[k, 3]
        for step in (0.25, 0.5):  # coverage steps about coverageTolerance = 0.25 (the guides keep their scale)
            k = pick()
            fa[k, 3] = np.where(fa[k, 3] >= f32(0.5), fa[k, 3] - f32(step), fa[k, 3] + f32(step))
        for value, plane, comp in ((np.nan, fn, 3), (np.inf, fn, 3), (-np.inf, fn, 1), (np.nan, fn, 0), (np.nan, fa, 3), (np.inf, fa, 3),
                                   (-1.0, fa, 3)):
            plane[rng.integers(0, n, max(1, n // 60)), comp] = value
        return alb, nd, obj

    frames = [frame(c) for c in [pcam] + cams]
    motion = np.zeros((3, N_IDS - 2, 4), f32)
    motion[:, :, :3] = (rng.standard_normal((3, N_IDS - 2, 3)) * 0.02).astype(f32)
    motion[:, 0, :3] = 0
    motion[:, :, 3] = np.array([0, 1, np.nan, 2.5], f32)[None, :N_IDS - 2]
    motion[1, 2, 0] = np.nan  # a table entry that is no number: its pixels do not project
    return dict(cameras=np.ascontiguousarray(np.stack(cams).astype(f32)), albedo=np.ascontiguousarray(np.stack([fr[0] for fr in frames[1:]])),
                nd=np.ascontiguousarray(np.stack([fr[1] for fr in frames[1:]])),
                objects=np.ascontiguousarray(np.stack([fr[2] for fr in frames[1:]])), motion=np.ascontiguousarray(motion),
                prev=(pcam,) + tuple(np.ascontiguousarray(a) for a in frames[0]))


FORMS = [dict(objects=False, table=False), dict(objects=True, table=False), dict(objects=True, table=True)]

__all__ = ["FORMS", "FlowChecker", "KINDS", "N_IDS", "SNAP", "TOLERANCES", "cameras_floats", "flow_frame_numpy", "flow_numpy",
           "synthetic_clip"]
