"""A clip whose camera orbits the scene (5 degrees per frame round the default look-at), 32 and 128 frames, animated (kFlagAnimate) and
static, with its denoiser planes (not progressive: every frame its own), three ways: (a) tptSetCamera + tptUpdate + tptDrawDeviceMoments
per frame, each frame into its own tile and planes (no copies, no synchronise between frames), (b) one tptDrawDeviceCameraClip call with
all four per-frame plane outputs and the cameras, (c) one tptDrawDeviceAnimationMoments call with the camera fixed (what a clip cost
before its camera could move: one launch per 32 frames while the scene moves, one per frame when it does not).  The modes run as
alternating brackets in one process: a bracket is as many clips as take at least --seconds, the host clock around work that ends in
tptSynchronize.  Prints one JSON line per (clip, mode, bracket) and one summary line per clip: median and range of ms per frame and
Gray/s, (b) / (a), (b) / (c), the kernel time per launch of (b) and (c), and whether (a) and (b) wrote the same bytes.
    python3 tools/camera_clip_rate.py [--brackets N] [--seconds S] [--frames 32,128] [--only 640x360|1280x720] [--scenes animated,static]"""
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

ANIMATE = 1  # kFlagAnimate (without kFlagProgressive)


def orbit(n, step=5.0):
    a = np.radians(step * np.arange(n))
    v = np.zeros((n, 9), np.float32)
    v[:, 0], v[:, 1], v[:, 2] = 3.0 * np.sin(a), 2.0, 3.0 * np.cos(a)
    v[:, 6], v[:, 7], v[:, 8] = 60.0, 0.02, 3.0
    return v


def planes(w, h, n):
    return torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")


class Mode:
    def __init__(self, w, h, n, flags):
        self.w, self.h, self.n, self.flags = w, h, n, flags
        self.times = [f / 60.0 for f in range(n)]  # a clip at 60 frames per second
        self.views = orbit(n)
        self.tile, self.mo = planes(w, h, 1), planes(w, h, 1)
        self.tiles, self.albedo, self.nd, self.moments = (planes(w, h, n) for _ in range(4))


class Sequence(Mode):
    """(a): the only way before"""
    def clip(self):
        w, h = self.w, self.h
        for j, t in enumerate(self.times):
            v = self.views[j]
            api.set_camera(v[0:3], v[3:6], float(v[6]), float(v[7]), float(v[8]))
            api.UpdateTest(t, j, w, h, self.flags)
            api.draw_device_moments(t, j, w, h, self.tiles[j].data_ptr(), self.moments[j].data_ptr(), self.flags,
                                    albedo_ptr=self.albedo[j].data_ptr(), normal_depth_ptr=self.nd[j].data_ptr())


class CameraClip(Mode):
    """(b): one call per clip"""
    def clip(self):
        api.draw_device_camera_clip(self.times, self.views, 0, self.w, self.h, self.tile.data_ptr(), self.mo.data_ptr(), self.flags,
                                    images_ptr=self.tiles.data_ptr(), albedo_ptr=self.albedo.data_ptr(), normal_depth_ptr=self.nd.data_ptr(),
                                    frame_moments_ptr=self.moments.data_ptr())


class FixedCamera(Mode):
    """(c): one call per clip, the camera of the clip's first frame throughout"""
    def clip(self):
        api.draw_device_animation_moments(self.times, 0, self.w, self.h, self.tile.data_ptr(), self.mo.data_ptr(), self.flags,
                                          images_ptr=self.tiles.data_ptr(), albedo_ptr=self.albedo.data_ptr(),
                                          normal_depth_ptr=self.nd.data_ptr(), frame_moments_ptr=self.moments.data_ptr())


def prepare(mode):
    api.set_camera(None)  # (the brackets alternate: (c) always renders through the default camera)
    api.UpdateTest(mode.times[0], 0, mode.w, mode.h, mode.flags)


def bracket(mode, reps):
    prepare(mode)
    api.synchronize()
    r0 = api.ray_counter_read()
    t0 = time.perf_counter()
    for _ in range(reps):
        mode.clip()
    api.synchronize()
    dt = time.perf_counter() - t0
    return api.ray_counter_read() - r0, dt


def clip(name, w, h, spp, n, flags, brackets, seconds):
    api.set_samples_per_pixel(spp)
    api.set_scene(None)
    modes = {"a_set_camera_update_draw_moments": Sequence(w, h, n, flags), "b_camera_clip": CameraClip(w, h, n, flags),
             "c_animation_moments_fixed_camera": FixedCamera(w, h, n, flags)}
    A, B, Cm = modes
    torch.cuda.synchronize()
    reps = {}
    for m, mode in modes.items():  # warm-up (buffers, code objects), then how many clips make a bracket
        bracket(mode, 1)
        _, dt = bracket(mode, 2)
        reps[m] = max(1, math.ceil(1.2 * seconds / (dt / 2)))
    ms, rate = {m: [] for m in modes}, {m: [] for m in modes}
    for b in range(brackets):
        for m, mode in modes.items():
            rays, dt = bracket(mode, reps[m])
            while dt < seconds:  # (a bracket that came out short is run again, longer)
                reps[m] *= 2
                rays, dt = bracket(mode, reps[m])
            ms[m].append(dt / (reps[m] * n) * 1e3)
            rate[m].append(rays / dt / 1e9)
            print(json.dumps(dict(config=name, mode=m, bracket=b, clips=reps[m], seconds=round(dt, 3), ms_per_frame=round(ms[m][-1], 4),
                                  gray_s=round(rate[m][-1], 3))), flush=True)
    a, b = modes[A], modes[B]
    torch.cuda.synchronize()
    same = {k: bool(torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32))) for k in ("tiles", "albedo", "nd", "moments")}
    kernel = {}
    for m in (B, Cm):
        prepare(modes[m])
        api.kernel_timing_begin(4 + n)
        modes[m].clip()
        kernel[m] = api.kernel_timing_end()
    api.set_camera(None)
    med = {m: statistics.median(v) for m, v in rate.items()}
    out = dict(config=name, w=w, h=h, spp=spp, frames_per_clip=n, animated=bool(flags & ANIMATE), brackets=brackets,
               median_ms_per_frame={m: round(statistics.median(v), 4) for m, v in ms.items()},
               range_ms_per_frame={m: [round(min(v), 4), round(max(v), 4)] for m, v in ms.items()},
               median_gray_s={m: round(v, 3) for m, v in med.items()},
               range_gray_s={m: [round(min(v), 3), round(max(v), 3)] for m, v in rate.items()},
               b_over_a=round(med[B] / med[A], 3), b_over_c=round(med[B] / med[Cm], 3), a_b_same_bytes=same,
               launches_per_call={m: k[1] for m, k in kernel.items()},
               kernel_ms_per_launch={m: round(k[0] / max(1, k[1]), 3) for m, k in kernel.items()}, pipeline=api.pipeline_info())
    print(json.dumps(out), flush=True)
    del modes, a, b
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5, help="shortest bracket")
    ap.add_argument("--frames", default="32,128", help="frames per clip, comma-separated")
    ap.add_argument("--only", default="", help="640x360 or 1280x720")
    ap.add_argument("--scenes", default="animated,static")
    args = ap.parse_args()
    api.InitializeTest()
    try:
        for w, h in ((640, 360), (1280, 720)):
            if args.only not in ("", "%dx%d" % (w, h)):
                continue
            for n in (int(x) for x in args.frames.split(",")):
                for scene in args.scenes.split(","):
                    clip("%dx%dx4 %d frames %s" % (w, h, n, scene), w, h, 4, n, ANIMATE if scene == "animated" else 0, args.brackets, args.seconds)
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
