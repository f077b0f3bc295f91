"""The cost and the use of tptObjectPlaneDevice and tptTemporalAccumulateObjectsDevice.
(1) Kernel time of the object plane at 1280x720 and 3840x2160 for the 46-sphere default scene and the 4096-sphere stress scene, beside
the five iterations of tptDenoiseDeviceVariance (a frame's a-trous chain) on the same frame's planes.
(2) Kernel time of the object-following pass against tptTemporalAccumulateDevice on the same traced planes: the first frame of a
sequence, a camera that stands still, one that orbits 0.5 degrees; with a table (46 entries, zero motion, no caps) and without one.
Both: tptTimerBegin / tptTimerEnd around --calls calls on the context stream, --reps alternating brackets (every variant once per
round, round after round), median / min / max.
(3) Quality on tools/temporal_rate.py's clips and definitions (4-spp frames, reference = the last frame at 1024 spp, squared error over
the raw last frame's, linear and relative; T = the pass alone, T+S = the pass in front of tptDenoiseDeviceVariance): the plain pass,
the pass following objects (tptObjectMotionTable's table), and that with caps of 1 and 2 on the metal and dielectric spheres.  Clips A,
B, C as there, and A-fast: A with time 0.3 j (spheres 1 and 8 move by several pixels per frame).  Every figure for the whole image and
for the pixels whose id is 1 or 8 in the last frame.  One JSON line per measurement.
    python3 tools/object_motion_rate.py [--calls N] [--reps R] [--only plane|pass|quality]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402
from toypathtracer_amd.scenes import STRESS_CAMERA, stress_scene  # noqa: E402

ANIMATE = 1


def plane(w, h):
    return torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")


def ids(w, h, n=1):
    return torch.zeros((n, h, w), dtype=torch.int32, device="cuda")


def orbit(j, degrees):
    a = math.radians(degrees * j)
    return dict(look_from=(3.0 * math.sin(a), 2.0, 3.0 * math.cos(a)), look_at=(0.0, 0.0, 0.0), vfov=60.0, aperture=0.02, focus_dist=3.0)


def trace(w, h, j, flags, time, camera):
    """frame j alone -> (camera record, [colour, albedo, nd, moments], object plane)"""
    api.set_camera(**camera)
    api.UpdateTest(time, j, w, h, flags)
    cam = api.GetSceneDesc()[2].copy()
    p = [plane(w, h) for _ in range(4)]
    obj = ids(w, h)
    torch.cuda.synchronize()
    api.draw_device_moments(time, j, w, h, p[0].data_ptr(), p[3].data_ptr(), flags, albedo_ptr=p[1].data_ptr(), normal_depth_ptr=p[2].data_ptr())
    api.object_plane_device(w, h, obj.data_ptr())
    return cam, p, obj[0]


def brackets(calls_of, calls, reps):
    """every variant once per round, `reps` rounds -> {name: [us per call]}"""
    for f in calls_of.values():
        f()
    api.synchronize()
    us = {k: [] for k in calls_of}
    for _ in range(reps):
        for k, f in calls_of.items():
            n = calls[k] if isinstance(calls, dict) else calls
            api.timer_begin()
            for _ in range(n):
                f()
            us[k].append(api.timer_end() / n * 1000)
    return us


def report(measure, us, reps, **more):
    med = {k: statistics.median(v) for k, v in us.items()}
    print(json.dumps(dict(measure=measure, reps=reps, us={k: round(v, 1) for k, v in med.items()},
                          range_us={k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()}, **more)), flush=True)
    return med


def plane_timing(calls, reps):
    for scene in ("default46", "stress4096"):
        if scene == "stress4096":
            api.set_scene(*stress_scene(4096, 64))
            camera = STRESS_CAMERA
        else:
            api.set_scene(None)
            camera = orbit(0, 0.0)
        for w, h in ((1280, 720), (3840, 2160)):
            cam, p, obj = trace(w, h, 0, 0, 0.0, camera)
            out, dst = ids(w, h), plane(w, h)
            api.synchronize()
            calls_of = {
                "object_plane": lambda: api.object_plane_device(w, h, out.data_ptr()),
                "atrous_5it": lambda: api.denoise_device_variance(w, h, p[0].data_ptr(), p[3].data_ptr(), 4.0, dst.data_ptr(),
                                                                  albedo_ptr=p[1].data_ptr(), normal_depth_ptr=p[2].data_ptr()),
            }
            n = {"object_plane": max(1, calls // 10) if scene == "stress4096" else calls, "atrous_5it": calls}
            med = report("object_plane_%s_%dx%d" % (scene, w, h), brackets(calls_of, n, reps), reps, calls=n,
                         spheres=api.scene_info()["spheres"], hit_share=round(float((obj >= 0).float().mean()), 4))
            print(json.dumps(dict(measure="object_plane_%s_%dx%d_ratio" % (scene, w, h),
                                  plane_over_atrous_chain=round(med["object_plane"] / med["atrous_5it"], 3),
                                  sphere_tests_per_ns=round(api.scene_info()["spheres"] * w * h / (med["object_plane"] * 1000), 2))), flush=True)
    api.set_scene(None)
    api.set_camera(None)


def pass_timing(calls, reps):
    api.set_scene(None)
    for w, h in ((1280, 720), (3840, 2160)):
        cam0, f0, o0 = trace(w, h, 0, 0, 0.0, orbit(0, 0.5))
        first = [plane(w, h) for _ in range(4)]
        api.temporal_accumulate_device(w, h, cam0, *[t.data_ptr() for t in f0], *[t.data_ptr() for t in first])
        prev = (cam0, first[0], first[1], f0[2], first[2])
        still = trace(w, h, 1, 0, 0.0, orbit(0, 0.5))
        moved = trace(w, h, 1, 0, 0.0, orbit(1, 0.5))
        outs = [plane(w, h) for _ in range(4)]
        table = torch.zeros((api.GetObjectCount()[0], 4), dtype=torch.float32, device="cuda")
        api.synchronize()
        po = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731

        def plain(frame, history):
            api.temporal_accumulate_device(w, h, frame[0], *po(frame[1]), *po(outs), max_history=64.0,
                                           prev=(prev[0],) + tuple(po(prev[1:])) if history else None)

        def objects(frame, history, with_table):
            api.temporal_accumulate_objects_device(w, h, frame[0], *po(frame[1]), frame[2].data_ptr(), *po(outs), max_history=64.0,
                                                   prev=(prev[0],) + tuple(po(prev[1:])) + (o0.data_ptr(),) if history else None,
                                                   motion_ptr=table.data_ptr() if with_table else None,
                                                   n_objects=table.shape[0] if with_table else 0)

        calls_of = {}
        for name, frame, history in (("first", (cam0, f0, o0), False), ("still", still, True), ("orbit", moved, True)):
            calls_of[name + "_plain"] = lambda frame=frame, history=history: plain(frame, history)
            calls_of[name + "_objects"] = lambda frame=frame, history=history: objects(frame, history, False)
            calls_of[name + "_objects_table"] = lambda frame=frame, history=history: objects(frame, history, True)
        med = report("object_pass_%dx%d" % (w, h), brackets(calls_of, calls, reps), reps, calls=calls)
        print(json.dumps(dict(measure="object_pass_%dx%d_ratio" % (w, h),
                              over_plain={k: round(med[k] / med[k.split("_")[0] + "_plain"], 3) for k in med if not k.endswith("_plain")})),
              flush=True)
    api.set_camera(None)


def figures(x, ref, mask=None):
    d = (x[..., :3].double() - ref) ** 2
    r = d / (ref ** 2 + 0.01)
    if mask is not None:
        d, r = d[mask], r[mask]
    return float(d.mean()), float(r.mean())


def spatial(w, h, colour, albedo, nd, moments):
    out = plane(w, h)
    api.denoise_device_variance(w, h, colour.data_ptr(), moments.data_ptr(), 4.0, out.data_ptr(), albedo_ptr=albedo.data_ptr(),
                                normal_depth_ptr=nd.data_ptr())
    api.synchronize()
    return out


CLIPS = {"A": (0.0, 16, 0.05), "B": (0.2, 16, 0.05), "C": (0.5, 12, 0.05), "A-fast": (0.0, 16, 0.3)}


def clip(name, w, h):
    degrees, frames, step = CLIPS[name]
    traced = [trace(w, h, j, ANIMATE, step * j, orbit(j, degrees)) for j in range(frames)]
    last = frames - 1
    api.set_samples_per_pixel(1024)
    ref = trace(w, h, last, ANIMATE, step * last, orbit(last, degrees))[1][0]
    api.synchronize()
    api.set_samples_per_pixel(4)
    ref = ref[..., :3].double()
    cur, obj = traced[last][1], traced[last][2]
    moving = (obj == 1) | (obj == 8)
    mats = api.GetSceneDesc()[1]
    glossy = mats["type"] != 0
    capped = torch.from_numpy(np.isin(obj.cpu().numpy(), np.nonzero(glossy)[0])).cuda()
    masks = {"image": None, "ids_1_8": moving, "metal_glass": capped}
    raw = {m: figures(cur[0], ref, mask) for m, mask in masks.items()}
    over = lambda x: {m: [round(v / r, 4) for v, r in zip(figures(x, ref, mask), raw[m])] for m, mask in masks.items()}  # noqa: E731
    print(json.dumps(dict(clip=name, size=[w, h], frames=frames, time_step=step, raw={m: list(v) for m, v in raw.items()},
                          pixels={m: int(w * h if mask is None else mask.sum()) for m, mask in masks.items()},
                          S=over(spatial(w, h, cur[0], cur[1], cur[2], cur[3])))), flush=True)
    for variant, cap in (("plain", None), ("ids", None), ("followed", 0.0), ("followed_cap2", 2.0), ("followed_cap1", 1.0)):
        prev = outs = None
        for j, (cam, p, o) in enumerate(traced):
            outs = [plane(w, h) for _ in range(4)]
            ptrs = [t.data_ptr() for t in p]
            if variant == "plain":
                api.temporal_accumulate_device(w, h, cam, *ptrs, *[t.data_ptr() for t in outs],
                                               prev=None if prev is None else (prev[0],) + tuple(t.data_ptr() for t in prev[1:5]))
            else:
                table = None
                if variant != "ids" and j > 0:  # (the first frame has no history to move)
                    t = api.object_motion_table(step * j, step * (j - 1), ANIMATE)
                    t[:, 3] = np.where(glossy, cap, 0.0)
                    table = torch.from_numpy(t).cuda()
                api.temporal_accumulate_objects_device(w, h, cam, *ptrs, o.data_ptr(), *[t.data_ptr() for t in outs],
                                                       prev=None if prev is None else (prev[0],) + tuple(t.data_ptr() for t in prev[1:]),
                                                       motion_ptr=None if table is None else table.data_ptr(),
                                                       n_objects=0 if table is None else table.shape[0])
                api.synchronize()  # (the table is this iteration's tensor)
            prev = (cam, outs[0], outs[1], p[2], outs[2], o)
        api.synchronize()
        N = outs[2][..., 3]
        print(json.dumps(dict(clip=name, size=[w, h], variant=variant, T=over(outs[0]),
                              TS=over(spatial(w, h, outs[0], outs[1], cur[2], outs[3])), mean_N=round(float(N.mean()), 3),
                              mean_N_ids_1_8=round(float(N[moving].mean()), 3) if bool(moving.any()) else None,
                              share_N1=round(float((N == 1).float().mean()), 4))), flush=True)


def quality():
    api.set_scene(None)
    for name, w, h in (("A", 640, 360), ("A-fast", 640, 360), ("A", 320, 180), ("A-fast", 320, 180), ("B", 320, 180), ("C", 320, 180)):
        clip(name, w, h)
    api.set_camera(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["plane", "pass", "quality"])
    a = ap.parse_args()
    api.InitializeTest()
    try:
        print(json.dumps(dict(device=api.device_name(), temporal_defaults=api.TEMPORAL_DEFAULTS,
                              variance_defaults=api.DENOISE_VARIANCE_DEFAULTS)), flush=True)
        if a.only in (None, "plane"):
            plane_timing(a.calls, a.reps)
        if a.only in (None, "pass"):
            pass_timing(a.calls, a.reps)
        if a.only in (None, "quality"):
            quality()
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
