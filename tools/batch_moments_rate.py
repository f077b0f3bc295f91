"""A progressive still with the planes tptDenoiseDeviceVariance reads -- 64 frames at 640x360x4 and 1280x720x4, the guide planes averaged
as the tile is -- three ways: (a) tptDrawDeviceMoments per frame, the guide planes blended with torch after each frame (the only way
before, tools/denoise_variance_rate.py), (b) one tptDrawDeviceCameraClip call with the camera repeated and per-frame guide planes, which
torch then folds, (c) one tptDrawDeviceBatchMoments call.  The ways run as alternating brackets in one process: a bracket is as many
stills as take at least --seconds, the host clock around work that ends in tptSynchronize (torch works on the context's stream).  Prints
one JSON line per (size, way, bracket) and one summary line per size: median and range of ms per frame and Gray/s, (c) / (a), (c) / (b),
and whether the three ways wrote the same tile and moments (the guides of (a) and (b) are torch's blend, not the library's, and are
compared by their largest difference).
    python3 tools/batch_moments_rate.py [--brackets N] [--seconds S] [--frames 64] [--only 640x360|1280x720]
    python3 tools/batch_moments_rate.py --once a|c --only 640x360     (one still, for a kernel trace: the fold beside the blends it replaces)"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402

PROGRESSIVE = api.kFlagProgressive
# the context's default camera (Test.cpp:309-319: the aperture is the float product 0.1f * 0.2f, not 0.02f)
DEFAULT_VIEW = [0.0, 2.0, 3.0, 0.0, 0.0, 0.0, 60.0, float(np.float32(0.1) * np.float32(0.2)), 3.0]


def planes(w, h, n=1):
    return torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")


class Way:
    def __init__(self, w, h, n):
        self.w, self.h, self.n = w, h, n
        self.tile, self.mo, self.albedo, self.nd = (planes(w, h)[0] for _ in range(4))
        self.lerp = [float(np.float32(f) / np.float32(f + 1)) for f in range(n)]

    def zero(self):
        for p in (self.tile, self.mo, self.albedo, self.nd):
            p.zero_()


class PerFrame(Way):
    """(a): a trace launch and two blends per frame, the guides blended by the caller"""
    def __init__(self, w, h, n):
        super().__init__(w, h, n)
        self.a_j, self.nd_j = planes(w, h)[0], planes(w, h)[0]

    def still(self):
        w, h = self.w, self.h
        for f in range(self.n):
            api.draw_device_moments(0.0, f, w, h, self.tile.data_ptr(), self.mo.data_ptr(), PROGRESSIVE, albedo_ptr=self.a_j.data_ptr(),
                                    normal_depth_ptr=self.nd_j.data_ptr())
            for avg, plane in ((self.albedo, self.a_j), (self.nd, self.nd_j)):
                avg.mul_(self.lerp[f]).add_(plane, alpha=1.0 - self.lerp[f])


class RepeatedCamera(Way):
    """(b): the camera-clip call with one camera for every frame, its per-frame guide planes folded by the caller"""
    def __init__(self, w, h, n):
        super().__init__(w, h, n)
        self.times = [0.0] * n
        self.views = np.float32([DEFAULT_VIEW] * n)
        self.frame_albedo, self.frame_nd = planes(w, h, n), planes(w, h, n)

    def still(self):
        api.draw_device_camera_clip(self.times, self.views, 0, self.w, self.h, self.tile.data_ptr(), self.mo.data_ptr(), PROGRESSIVE,
                                    albedo_ptr=self.frame_albedo.data_ptr(), normal_depth_ptr=self.frame_nd.data_ptr(), cameras=False)
        for f in range(self.n):
            for avg, stack in ((self.albedo, self.frame_albedo), (self.nd, self.frame_nd)):
                avg.mul_(self.lerp[f]).add_(stack[f], alpha=1.0 - self.lerp[f])


class BatchMoments(Way):
    """(c): one call"""
    def still(self):
        api.draw_device_batch_moments(0.0, 0, self.n, self.w, self.h, self.tile.data_ptr(), self.mo.data_ptr(), PROGRESSIVE,
                                      albedo_ptr=self.albedo.data_ptr(), normal_depth_ptr=self.nd.data_ptr())


def bracket(way, reps):
    api.set_camera(None)
    api.UpdateTest(0.0, 0, way.w, way.h, PROGRESSIVE)
    way.zero()
    torch.cuda.synchronize()
    api.synchronize()
    r0 = api.ray_counter_read()
    t0 = time.perf_counter()
    for _ in range(reps):
        way.still()
    api.synchronize()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return api.ray_counter_read() - r0, dt


def size(w, h, spp, n, brackets, seconds):
    name = "%dx%dx%d %d progressive frames" % (w, h, spp, n)
    api.set_samples_per_pixel(spp)
    api.set_scene(None)
    ways = {"a_draw_moments_per_frame_torch_guides": PerFrame(w, h, n), "b_camera_clip_repeated_camera_torch_fold": RepeatedCamera(w, h, n),
            "c_batch_moments": BatchMoments(w, h, n)}
    A, B, Cw = ways
    reps = {}
    for m, way in ways.items():  # warm-up (buffers, code objects), then how many stills make a bracket
        bracket(way, 1)
        _, dt = bracket(way, 2)
        reps[m] = max(1, math.ceil(1.2 * seconds / (dt / 2)))
    ms, rate = {m: [] for m in ways}, {m: [] for m in ways}
    for b in range(brackets):
        for m, way in ways.items():
            rays, dt = bracket(way, reps[m])
            while dt < seconds:  # (a bracket that came out short is run again, longer)
                reps[m] *= 2
                rays, dt = bracket(way, reps[m])
            ms[m].append(dt / (reps[m] * n) * 1e3)
            rate[m].append(rays / dt / 1e9)
            print(json.dumps(dict(config=name, way=m, bracket=b, stills=reps[m], seconds=round(dt, 3), ms_per_frame=round(ms[m][-1], 4),
                                  gray_s=round(rate[m][-1], 3))), flush=True)
    for way in ways.values():  # one still each on zeroed planes: what they wrote
        bracket(way, 1)
    same = {m: {k: bool(torch.equal(getattr(ways[Cw], k).view(torch.int32), getattr(ways[m], k).view(torch.int32))) for k in ("tile", "mo")}
            for m in (A, B)}
    guide_diff = {m: max(float((getattr(ways[Cw], k) - getattr(ways[m], k)).abs().max()) for k in ("albedo", "nd")) for m in (A, B)}
    med = {m: statistics.median(v) for m, v in rate.items()}
    out = dict(config=name, w=w, h=h, spp=spp, frames=n, brackets=brackets,
               median_ms_per_frame={m: round(statistics.median(v), 4) for m, v in ms.items()},
               range_ms_per_frame={m: [round(min(v), 4), round(max(v), 4)] for m, v in ms.items()},
               median_gray_s={m: round(v, 3) for m, v in med.items()},
               range_gray_s={m: [round(min(v), 3), round(max(v), 3)] for m, v in rate.items()},
               c_over_a=round(med[Cw] / med[A], 3), c_over_b=round(med[Cw] / med[B], 3), tile_and_moments_same_bytes_as_c=same,
               largest_guide_difference_from_c=guide_diff, pipeline=api.pipeline_info())
    print(json.dumps(out), flush=True)
    del ways
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--brackets", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.5, help="shortest bracket")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--only", default="", help="640x360 or 1280x720")
    ap.add_argument("--once", default="", help="a, b or c: one warm-up still and one still of that way, nothing timed")
    args = ap.parse_args()
    api.InitializeTest()
    try:
        for w, h in ((640, 360), (1280, 720)):
            if args.only not in ("", "%dx%d" % (w, h)):
                continue
            if args.once:
                api.set_samples_per_pixel(4)
                way = {"a": PerFrame, "b": RepeatedCamera, "c": BatchMoments}[args.once](w, h, args.frames)
                for _ in range(2):
                    bracket(way, 1)
                print(json.dumps(dict(once=args.once, w=w, h=h, frames=args.frames)))
            else:
                size(w, h, 4, args.frames, args.brackets, args.seconds)
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
