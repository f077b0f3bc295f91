"""An animated clip of 32 frames (--frames-per-call) with its denoiser planes (kFlagAnimate, not progressive: every frame its own), three ways: (a) tptUpdate +
tptDrawDeviceMoments per frame, each frame into its own tile and planes (no copies, no synchronise between frames), (b) one
tptDrawDeviceAnimationMoments call with all four per-frame plane outputs, (c) tptDrawDeviceAnimation with its frame images (the colour
alone).  The modes run as alternating brackets in one process: a bracket is as many clips as take at least --seconds, the host clock
around work that ends in tptSynchronize.  Prints one JSON line per (size, mode, bracket) and one summary line per size: median and range
of ms per frame and Gray/s, (b) / (a), (b) / (c), the kernel time of one call's launches, and whether (a) and (b) wrote the same bytes.
--frames-per-call above 32 shows what a longer call gains: its launches overlap, where separate calls are ordered on the context stream.
    python3 tools/animation_moments_rate.py [--brackets N] [--seconds S] [--frames-per-call F] [--only 640x360|1280x720]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402

ANIMATE = 1  # kFlagAnimate (without kFlagProgressive)
N = 32   # frames per call (--frames-per-call)
TIMES = []  # their times: a clip at 60 frames per second


def planes(w, h, n=None):
    return torch.zeros((n or N, h, w, 4), dtype=torch.float32, device="cuda")


class Sequence:
    """(a): the parent's way"""
    def __init__(self, w, h):
        self.tiles, self.albedo, self.nd, self.moments = (planes(w, h) for _ in range(4))

    def clip(self, w, h):
        for j, t in enumerate(TIMES):
            api.UpdateTest(t, j, w, h, ANIMATE)
            api.draw_device_moments(t, j, w, h, self.tiles[j].data_ptr(), self.moments[j].data_ptr(), ANIMATE,
                                    albedo_ptr=self.albedo[j].data_ptr(), normal_depth_ptr=self.nd[j].data_ptr())


class Clip:
    """(b): one call per clip"""
    def __init__(self, w, h):
        self.tile, self.mo = planes(w, h, 1), planes(w, h, 1)
        self.tiles, self.albedo, self.nd, self.moments = (planes(w, h) for _ in range(4))

    def clip(self, w, h):
        api.draw_device_animation_moments(TIMES, 0, w, h, self.tile.data_ptr(), self.mo.data_ptr(), ANIMATE, images_ptr=self.tiles.data_ptr(),
                                          albedo_ptr=self.albedo.data_ptr(), normal_depth_ptr=self.nd.data_ptr(),
                                          frame_moments_ptr=self.moments.data_ptr())


class Colour:
    """(c): the colour alone"""
    def __init__(self, w, h):
        self.tile, self.tiles = planes(w, h, 1), planes(w, h)

    def clip(self, w, h):
        api.draw_device_animation(TIMES, 0, w, h, self.tile.data_ptr(), ANIMATE, self.tiles.data_ptr())


def bracket(mode, w, h, reps):
    api.UpdateTest(TIMES[0], 0, w, h, ANIMATE)
    api.synchronize()
    r0 = api.ray_counter_read()
    t0 = time.perf_counter()
    for _ in range(reps):
        mode.clip(w, h)
    api.synchronize()
    dt = time.perf_counter() - t0
    return api.ray_counter_read() - r0, dt


def size(name, w, h, spp, brackets, seconds):
    api.set_samples_per_pixel(spp)
    api.set_scene(None)
    modes = {"a_update_draw_moments": Sequence(w, h), "b_animation_moments": Clip(w, h), "c_animation": Colour(w, h)}
    torch.cuda.synchronize()
    reps = {}
    for m, mode in modes.items():  # warm-up (buffers, code objects), then how many clips make a bracket
        bracket(mode, w, h, 2)
        _, dt = bracket(mode, w, h, 4)
        reps[m] = max(1, math.ceil(1.2 * seconds / (dt / 4)))
    ms, rate = {m: [] for m in modes}, {m: [] for m in modes}
    for b in range(brackets):
        for m, mode in modes.items():
            rays, dt = bracket(mode, w, h, reps[m])
            while dt < seconds:  # (a bracket that came out short is run again, longer)
                reps[m] *= 2
                rays, dt = bracket(mode, w, h, reps[m])
            ms[m].append(dt / (reps[m] * N) * 1e3)
            rate[m].append(rays / dt / 1e9)
            print(json.dumps(dict(config=name, mode=m, bracket=b, clips=reps[m], seconds=round(dt, 3), ms_per_frame=round(ms[m][-1], 4),
                                  gray_s=round(rate[m][-1], 3))), flush=True)
    a, b = modes["a_update_draw_moments"], modes["b_animation_moments"]
    torch.cuda.synchronize()
    same = {k: bool(torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32))) for k in ("tiles", "albedo", "nd", "moments")}
    kernel = {}
    for m in ("b_animation_moments", "c_animation"):
        api.UpdateTest(TIMES[0], 0, w, h, ANIMATE)
        api.kernel_timing_begin(4 + N // 32)
        modes[m].clip(w, h)
        kernel[m] = api.kernel_timing_end()
    med = {m: statistics.median(v) for m, v in rate.items()}
    out = dict(config=name, w=w, h=h, spp=spp, frames_per_clip=N, brackets=brackets,
               median_ms_per_frame={m: round(statistics.median(v), 4) for m, v in ms.items()},
               range_ms_per_frame={m: [round(min(v), 4), round(max(v), 4)] for m, v in ms.items()},
               median_gray_s={m: round(v, 3) for m, v in med.items()},
               range_gray_s={m: [round(min(v), 3), round(max(v), 3)] for m, v in rate.items()},
               b_over_a=round(med["b_animation_moments"] / med["a_update_draw_moments"], 3),
               b_over_c=round(med["b_animation_moments"] / med["c_animation"], 3),
               a_b_same_bytes=same, kernel_ms_per_call={m: round(k[0], 3) for m, k in kernel.items()},
               launches_per_call={m: k[1] for m, k in kernel.items()}, pipeline=api.pipeline_info())
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5, help="shortest bracket")
    ap.add_argument("--frames-per-call", type=int, default=32)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    global N
    N = args.frames_per_call
    TIMES[:] = [f / 60.0 for f in range(N)]
    api.InitializeTest()
    try:
        if args.only in ("", "640x360"):
            size("640x360x4", 640, 360, 4, args.brackets, args.seconds)
        if args.only in ("", "1280x720"):
            size("1280x720x4", 1280, 720, 4, args.brackets, args.seconds)
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
