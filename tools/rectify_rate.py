"""The cost and the use of tptRectifyHistoryDevice.
(1) Time of the pass at 1280x720 and 3840x2160, radius 1..3, on traced planes behind tptTemporalAccumulateDevice (camera still, the
history found) -- interleaved in one process with that temporal pass and with ONE iteration of tptDenoiseDevice on the same planes:
tptTimerBegin / tptTimerEnd around --calls calls on the context stream, --reps alternating brackets, median / min / max.
(2) Quality of pass + rectification + tptDenoiseDeviceVariance against pass + filter (api.DENOISE_VARIANCE_DEFAULTS, demodulated,
samples = 4) on tools/temporal_rate.py's clips of 4-spp frames at 320x180 -- A static camera, kFlagAnimate, time 0.05 j, 16 frames;
B = A + an orbit of 0.2 degrees per frame; C = 0.5 degrees per frame, 12 frames; static = nothing moves, 12 frames -- and on the light
switch (96x54 and 320x180: seven frames with the emissive materials dark, then tptSetScene switches them on): max_history 4 / 8 / 16,
gamma 0.5 / 1 / 2 / 4, radius 1..3.  Reference = the last frame at 1024 spp; squared error over the raw last frame's, linear and
relative (mean((x - ref)^2 / (ref^2 + 0.01))): TS = pass + filter, TRS = pass + rectification + filter.
(3) --cpu-switch: the light switch, then clip A and the static clip, at 96x54 through the CPU statements of the whole chain
(tests/moments_checker.c, temporal_checker.c, rectify_checker.c, variance_checker.c) -- no GPU; the light switch's are the figures
tests/test_gpu_rectify.py's quality test rests on.
One JSON line per measurement.
    python3 tools/rectify_rate.py [--calls N] [--reps R] [--only timing|quality] | --cpu-switch"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANIMATE = 1
HISTORIES, GAMMAS, RADII = (4.0, 8.0, 16.0), (0.5, 1.0, 2.0, 4.0), (1, 2, 3)
SWITCH_FRAMES = 8


def cpu_switch():
    import tempfile

    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from moments_lib import DEMODULATE, MomentsChecker, VarianceChecker
    from oracle_lib import Oracle
    from rectify_lib import RectifyChecker
    from temporal_lib import TemporalChecker
    from toypathtracer_amd import api

    d = tempfile.mkdtemp()
    mc, vc, tc, rc = MomentsChecker(d), VarianceChecker(d), TemporalChecker(d), RectifyChecker(d)
    o = Oracle.get()
    w, h, spp = 96, 54, 4
    spheres, mats = o.default_scene()
    cam = o.default_camera(w, h)
    dark = mats.copy()
    dark["emissive"] = 0

    def figures(x, ref):
        dd = (x[..., :3].astype(np.float64) - ref) ** 2
        return float(dd.mean()), float((dd / (ref ** 2 + 0.01)).mean())

    def clip(name, frames, animate):
        """switch: the emissive materials dark until the last frame; A: kFlagAnimate, time 0.05 j; static: nothing moves"""
        traced = []
        for j in range(frames):
            sp = spheres.copy()
            if animate:
                o.animate(sp, 0.05 * j)
            m = dark if name == "switch" and j < frames - 1 else mats
            _, bb, mo, alb, nd = mc.render(sp, m, cam, w, h, spp, j, flags=0)
            traced.append((bb, alb, nd, mo))
        ref = mc.render(sp, mats, cam, w, h, 1024, frames - 1, flags=0)[1][..., :3].astype(np.float64)
        raw = figures(traced[-1][0], ref)

        def chain(max_history, rect):
            prev = None
            for cur in traced:
                oc, oa, om, ov = tc.run(cam, cur, prev, max_history=max_history)
                if rect:
                    oc, om, ov = rc.run(cur[0], cur[3], oc, om, **rect)
                prev = (cam, oc, oa, cur[2], om)
            out = vc.run(oc, oa, cur[2], ov, float(spp), flags=DEMODULATE, **api.DENOISE_VARIANCE_DEFAULTS)
            return [round(v, 5) for v in figures(out, ref)], round(float(om[..., 3].mean()), 3)

        label = name + " (CPU statements)"
        print(json.dumps(dict(clip=label, size=[w, h], frames=frames, mse_raw=raw[0], rel_raw=raw[1])), flush=True)
        for mh in HISTORIES:
            ts, n = chain(mh, None)
            print(json.dumps(dict(clip=label, max_history=mh, TS_abs=ts, mean_N=n)), flush=True)
            for r in RADII:
                for g in GAMMAS:
                    trs, n = chain(mh, dict(radius=r, gamma=g))
                    print(json.dumps(dict(clip=label, max_history=mh, radius=r, gamma=g, TRS_abs=trs, mean_N=n,
                                          TS_over_TRS=[round(a / b, 2) for a, b in zip(ts, trs)])), flush=True)

    clip("switch", SWITCH_FRAMES, False)
    clip("A", 16, True)
    clip("static", 12, False)


def gpu(a):
    import torch

    from toypathtracer_amd import api

    def plane(w, h):
        return torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")

    def orbit(j, degrees):
        t = math.radians(degrees * j)
        return dict(look_from=(3.0 * math.sin(t), 2.0, 3.0 * math.cos(t)), look_at=(0.0, 0.0, 0.0), vfov=60.0, aperture=0.02, focus_dist=3.0)

    def trace(w, h, j, flags, time, camera):
        """frame j alone -> (camera record, [colour, albedo, nd, moments])"""
        api.set_camera(**camera)
        api.UpdateTest(time, j, w, h, flags)
        cam = api.GetSceneDesc()[2].copy()
        p = [plane(w, h) for _ in range(4)]
        torch.cuda.synchronize()
        api.draw_device_moments(time, j, w, h, p[0].data_ptr(), p[3].data_ptr(), flags, albedo_ptr=p[1].data_ptr(), normal_depth_ptr=p[2].data_ptr())
        return cam, p

    def accumulate(w, h, cam, cur, prev, outs=None, **kw):
        outs = outs or [plane(w, h) for _ in range(4)]
        api.temporal_accumulate_device(w, h, cam, *[t.data_ptr() for t in cur], *[t.data_ptr() for t in outs],
                                       prev=None if prev is None else (prev[0],) + tuple(t.data_ptr() for t in prev[1:]), **kw)
        return outs

    def rectify(w, h, cur, acc, outs=None, **kw):
        outs = outs or [plane(w, h) for _ in range(3)]
        api.rectify_history_device(w, h, cur[0].data_ptr(), cur[3].data_ptr(), acc[0].data_ptr(), acc[2].data_ptr(),
                                   *[t.data_ptr() for t in outs], **kw)
        return outs

    def timing(calls, reps):
        for w, h in ((1280, 720), (3840, 2160)):
            cam0, f0 = trace(w, h, 0, 0, 0.0, orbit(0, 0.5))
            first = accumulate(w, h, cam0, f0, None)
            prev = (cam0, first[0], first[1], f0[2], first[2])
            cam1, f1 = trace(w, h, 1, 0, 0.0, orbit(0, 0.5))
            acc = accumulate(w, h, cam1, f1, prev, max_history=16.0)
            outs4, outs3 = [plane(w, h) for _ in range(4)], [plane(w, h) for _ in range(3)]
            api.synchronize()
            calls_of = {"rectify_r%d" % r: (lambda r=r: rectify(w, h, f1, acc, outs3, radius=r, gamma=1.0)) for r in RADII}
            calls_of["temporal_still"] = lambda: accumulate(w, h, cam1, f1, prev, outs4, max_history=16.0)
            calls_of["atrous_1it"] = lambda: api.denoise_device(w, h, f1[0].data_ptr(), outs4[0].data_ptr(), albedo_ptr=f1[1].data_ptr(),
                                                                normal_depth_ptr=f1[2].data_ptr(), iterations=1)
            for f in calls_of.values():
                f()
            api.synchronize()
            clipped = round(float((outs3[0] != acc[0]).any(dim=-1).float().mean()), 4)
            ms = {k: [] for k in calls_of}
            for _ in range(reps):
                for k, f in calls_of.items():
                    api.timer_begin()
                    for _ in range(calls):
                        f()
                    ms[k].append(api.timer_end() / calls * 1000)
            med = {k: statistics.median(v) for k, v in ms.items()}
            print(json.dumps(dict(measure="rectify_%dx%d" % (w, h), calls=calls, reps=reps, us={k: round(v, 1) for k, v in med.items()},
                                  range_us={k: [round(min(v), 1), round(max(v), 1)] for k, v in ms.items()},
                                  ratio_to_temporal={k: round(med[k] / med["temporal_still"], 3) for k in med if k.startswith("rectify")},
                                  ratio_to_atrous={k: round(med[k] / med["atrous_1it"], 3) for k in med if k.startswith("rectify")},
                                  share_clipped_r3=clipped)), flush=True)
        api.set_camera(None)

    def figures(x, ref):
        d = (x[..., :3].double() - ref) ** 2
        return float(d.mean()), float((d / (ref ** 2 + 0.01)).mean())

    def spatial(w, h, colour, albedo, nd, moments):
        out = plane(w, h)
        api.denoise_device_variance(w, h, colour.data_ptr(), moments.data_ptr(), 4.0, out.data_ptr(), albedo_ptr=albedo.data_ptr(),
                                    normal_depth_ptr=nd.data_ptr())
        api.synchronize()
        return out

    CLIPS = {"A": (0.0, 16, ANIMATE), "B": (0.2, 16, ANIMATE), "C": (0.5, 12, ANIMATE), "static": (0.0, 12, 0), "switch": (0.0, SWITCH_FRAMES, 0)}

    def clip(name, w, h):
        degrees, frames, flags = CLIPS[name]
        last = frames - 1
        spheres, mats, _, _ = api.GetSceneDesc()
        dark = mats.copy()
        dark["emissive"] = 0
        traced = []
        for j in range(frames):
            if name == "switch":
                api.set_scene(spheres, dark if j < last else mats)
            traced.append(trace(w, h, j, flags, 0.05 * j if flags else 0.0, orbit(j, degrees)))
        api.set_samples_per_pixel(1024)
        ref = trace(w, h, last, flags, 0.05 * last if flags else 0.0, orbit(last, degrees))[1][0]
        api.synchronize()
        api.set_samples_per_pixel(4)
        if name == "switch":
            api.set_scene(None)
        ref = ref[..., :3].double()
        cur = traced[last][1]
        raw = figures(cur[0], ref)
        over = lambda x: [round(v / r, 4) for v, r in zip(figures(x, ref), raw)]  # noqa: E731
        print(json.dumps(dict(clip=name, size=[w, h], frames=frames, mse_raw=raw[0], rel_raw=raw[1],
                              S=over(spatial(w, h, cur[0], cur[1], cur[2], cur[3])))), flush=True)

        def chain(mh, rect):
            prev = None
            for cam, p in traced:
                acc = accumulate(w, h, cam, p, prev, max_history=mh)
                colour, moments, variance = rectify(w, h, p, acc, **rect) if rect else (acc[0], acc[2], acc[3])
                prev = (cam, colour, acc[1], p[2], moments)
            api.synchronize()
            return over(spatial(w, h, colour, acc[1], cur[2], variance)), round(float(moments[..., 3].mean()), 3)

        for mh in HISTORIES:
            ts, n = chain(mh, None)
            print(json.dumps(dict(clip=name, size=[w, h], max_history=mh, TS=ts, mean_N=n)), flush=True)
            for r in RADII:
                row = {}
                for g in GAMMAS:
                    trs, n = chain(mh, dict(radius=r, gamma=g))
                    row["g%g" % g] = dict(TRS=trs, mean_N=n)
                print(json.dumps(dict(clip=name, size=[w, h], max_history=mh, radius=r, **row)), flush=True)

    def quality():
        for name, w, h in (("A", 320, 180), ("B", 320, 180), ("C", 320, 180), ("static", 320, 180), ("switch", 96, 54), ("switch", 320, 180)):
            clip(name, w, h)
        api.set_camera(None)

    api.InitializeTest()
    try:
        print(json.dumps(dict(device=api.device_name(), rectify_defaults=api.RECTIFY_DEFAULTS, temporal_defaults=api.TEMPORAL_DEFAULTS,
                              variance_defaults=api.DENOISE_VARIANCE_DEFAULTS)), flush=True)
        if a.only in (None, "timing"):
            timing(a.calls, a.reps)
        if a.only in (None, "quality"):
            quality()
    finally:
        api.ShutdownTest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["timing", "quality"])
    ap.add_argument("--cpu-switch", action="store_true")
    a = ap.parse_args()
    if a.cpu_switch:
        cpu_switch()
    else:
        gpu(a)


if __name__ == "__main__":
    main()
