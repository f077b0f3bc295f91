"""The cost and the use of tptTemporalAccumulateDevice.
(1) Kernel time of the pass at 1280x720 and 3840x2160 on traced planes -- the first frame of a sequence (no history), a camera that stands
still (one tap per pixel) and one that orbits 0.5 degrees (four taps) -- interleaved in one process with ONE iteration of
tptDenoiseDevice on the same planes (both guides, demodulated): tptTimerBegin / tptTimerEnd around --calls calls on the context
stream, --reps alternating brackets, median / min / max.
(2) Quality of the pass in front of tptDenoiseDeviceVariance (api.DENOISE_VARIANCE_DEFAULTS, demodulated, samples = 4) on clips of 4-spp
frames, reference = the last frame at 1024 spp with its own camera and time; squared error over the raw last frame's, linear and
relative (mean((x - ref)^2 / (ref^2 + 0.01))): S = the filter alone, T = the pass alone, T+S = pass then filter, blind = the
reference's own smoothing (the kFlagProgressive | kFlagAnimate tile of the same frames).  Clips: A static camera, kFlagAnimate, time
0.05 j, 16 frames (640x360 and 320x180); B = A + an orbit of 0.2 degrees per frame; C = 0.5 degrees per frame, 12 frames; static =
nothing moves, 12 frames.  With --sweep: max_history 2..16 for every clip, and the tolerances around api.TEMPORAL_DEFAULTS on A and B.
One JSON line per measurement.
    python3 tools/temporal_rate.py [--calls N] [--reps R] [--sweep] [--only timing|quality]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402

ANIMATE, PROGRESSIVE = 1, 2
TD = api.TEMPORAL_DEFAULTS


def plane(w, h):
    return torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")


def orbit(j, degrees):
    a = math.radians(degrees * j)
    return dict(look_from=(3.0 * math.sin(a), 2.0, 3.0 * math.cos(a)), look_at=(0.0, 0.0, 0.0), vfov=60.0, aperture=0.02, focus_dist=3.0)


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


def timing(calls, reps):
    for w, h in ((1280, 720), (3840, 2160)):
        cam0, f0 = trace(w, h, 0, 0, 0.0, orbit(0, 0.5))
        first = accumulate(w, h, cam0, f0, None)
        prev = (cam0, first[0], first[1], f0[2], first[2])
        still = trace(w, h, 1, 0, 0.0, orbit(0, 0.5))
        moved = trace(w, h, 1, 0, 0.0, orbit(1, 0.5))
        outs = [plane(w, h) for _ in range(4)]
        api.synchronize()
        calls_of = {
            "first": lambda: accumulate(w, h, cam0, f0, None, outs),
            "still": lambda: accumulate(w, h, still[0], still[1], prev, outs, max_history=64.0),
            "orbit": lambda: accumulate(w, h, moved[0], moved[1], prev, outs, max_history=64.0),
            "atrous_1it": lambda: api.denoise_device(w, h, f0[0].data_ptr(), outs[0].data_ptr(), albedo_ptr=f0[1].data_ptr(),
                                                     normal_depth_ptr=f0[2].data_ptr(), iterations=1),
        }
        share = {}
        for k in ("still", "orbit"):
            calls_of[k]()
            api.synchronize()
            share[k] = round(float((outs[2][..., 3] > 1).float().mean()), 4)
        for f in calls_of.values():
            f()
        api.synchronize()
        ms = {k: [] for k in calls_of}
        for _ in range(reps):
            for k, f in calls_of.items():
                api.timer_begin()
                for _ in range(calls):
                    f()
                ms[k].append(api.timer_end() / calls * 1000)
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps(dict(measure="temporal_%dx%d" % (w, h), calls=calls, reps=reps,
                              us={k: round(v, 1) for k, v in med.items()},
                              range_us={k: [round(min(v), 1), round(max(v), 1)] for k, v in ms.items()},
                              ratio_to_atrous={k: round(med[k] / med["atrous_1it"], 3) for k in ("first", "still", "orbit")},
                              share_with_history=share)), flush=True)
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


CLIPS = {"A": (0.0, 16, ANIMATE), "B": (0.2, 16, ANIMATE), "C": (0.5, 12, ANIMATE), "static": (0.0, 12, 0)}


def clip(name, w, h, sweeps):
    degrees, frames, flags = CLIPS[name]
    traced = [trace(w, h, j, flags, 0.05 * j, orbit(j, degrees)) for j in range(frames)]
    last = frames - 1
    api.set_samples_per_pixel(1024)
    ref = trace(w, h, last, flags, 0.05 * last, orbit(last, degrees))[1][0]
    api.synchronize()
    api.set_samples_per_pixel(4)
    ref = ref[..., :3].double()
    cur = traced[last][1]
    raw = figures(cur[0], ref)
    over = lambda x: [round(v / r, 4) for v, r in zip(figures(x, ref), raw)]  # noqa: E731
    # the reference's own temporal tool: the progressive tile with its animate smoothing
    tile = plane(w, h)
    for j in range(frames):
        api.set_camera(**orbit(j, degrees))
        api.UpdateTest(0.05 * j, j, w, h, flags | PROGRESSIVE)
        api.draw_device(0.05 * j, j, w, h, tile.data_ptr(), flags | PROGRESSIVE)
    api.synchronize()
    print(json.dumps(dict(clip=name, size=[w, h], frames=frames, mse_raw=raw[0], rel_raw=raw[1],
                          S=over(spatial(w, h, cur[0], cur[1], cur[2], cur[3])), blind=over(tile))), flush=True)
    for kw in sweeps:
        prev = outs = None
        for cam, p in traced:
            outs = accumulate(w, h, cam, p, prev, **kw)
            prev = (cam, outs[0], outs[1], p[2], outs[2])
        api.synchronize()
        N = outs[2][..., 3]
        print(json.dumps(dict(clip=name, size=[w, h], **dict(TD, **kw), T=over(outs[0]),
                              TS=over(spatial(w, h, outs[0], outs[1], cur[2], outs[3])), mean_N=round(float(N.mean()), 3),
                              share_N1=round(float((N == 1).float().mean()), 4))), flush=True)


def quality(sweep):
    histories = [dict(max_history=float(m)) for m in ((2, 3, 4, 6, 8, 16) if sweep else (4,))]
    tolerances = [dict(depth_tolerance=d, normal_tolerance=n, coverage_tolerance=c)
                  for d, n, c in ((0.02, 0.25, 0.0), (0.5, 0.25, 0.0), (0.1, 0.05, 0.0), (0.1, 1.0, 0.0), (0.1, 0.25, 0.25), (0.1, 0.25, 1.0))]
    for name, w, h in (("A", 640, 360), ("A", 320, 180), ("B", 320, 180), ("C", 320, 180), ("static", 320, 180)):
        clip(name, w, h, histories + (tolerances if sweep and name in ("A", "B") else []))
    api.set_camera(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--only", choices=["timing", "quality"])
    a = ap.parse_args()
    api.InitializeTest()
    try:
        print(json.dumps(dict(device=api.device_name(), temporal_defaults=TD, variance_defaults=api.DENOISE_VARIANCE_DEFAULTS)), flush=True)
        if a.only in (None, "timing"):
            timing(a.calls, a.reps)
        if a.only in (None, "quality"):
            quality(a.sweep)
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
