"""A clip whose spheres the CALLER moves while the camera orbits the scene (5 degrees per frame), 32 and 128 frames, with its denoiser
planes (not progressive: every frame its own): (a) tptSetScene + tptSetCamera + tptUpdate + tptDrawDeviceMoments per frame, each frame
into its own tile and planes (no copies, no synchronise between frames) -- the only way before, and unchanged code; (b) one
tptDrawDeviceCameraClip call with kFlagAnimate (the library's own motion of spheres 1 and 8); (c) one tptDrawDeviceKeyframeClip call
with 0, 2, 4 and 8 moved spheres -- with 2 they are spheres 1 and 8 at the centres (b) gives them, 4 and 8 add spheres that swing by up
to 0.3 about their places; (a) moves the eight.  Every variant runs once per round between tptTimerBegin and tptTimerEnd, as many clips
as took at least --seconds at warm-up; the figures are medians over the rounds.  Prints one JSON line per (clip, variant, round) and one
summary line per clip: median and range of ms per frame and Gray/s, (c) / (a), the slope of (c) over the number of moved spheres, the
launches and the kernel time per launch, and whether (a) and (c) with the same motion wrote the same bytes.
    python3 tools/keyframe_clip_rate.py [--rounds N] [--seconds S] [--frames 32,128] [--only 640x360|1280x720]"""
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

ANIMATE = 1  # kFlagAnimate (without kFlagProgressive)
IDS = [1, 8, 3, 7, 2, 4, 5, 6]


def orbit(n, step=5.0):
    a = np.radians(step * np.arange(n))
    v = np.zeros((n, 9), np.float32)
    v[:, 0], v[:, 1], v[:, 2] = 3.0 * np.sin(a), 2.0, 3.0 * np.cos(a)
    v[:, 6], v[:, 7], v[:, 8] = 60.0, 0.02, 3.0
    return v


def planes(w, h, n):
    return torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")


def motion(times, w, h):
    """-> (the default scene, float32 (n, 8, 3): spheres 1 and 8 where tptUpdate puts them at each time, the others swinging about
    their places)"""
    api.set_scene(None)
    n = len(times)
    c = np.zeros((n, len(IDS), 3), np.float32)
    for j, t in enumerate(times):
        api.UpdateTest(t, j, w, h, ANIMATE)
        s = api.GetSceneDesc()[0]
        for k, i in enumerate(IDS):
            c[j, k] = (s["cx"][i], s["cy"][i], s["cz"][i])
            if k >= 2:
                c[j, k] += np.float32(0.3) * np.float32([np.sin(3.0 * t + k), 0.0, np.cos(2.0 * t + k)])
    api.set_scene(None)
    api.UpdateTest(times[0], 0, w, h, 0)
    scene = api.GetSceneDesc()[:2]
    return (scene[0].copy(), scene[1].copy()), c


class Mode:
    def __init__(self, w, h, n, flags, scene, centres, moved):
        self.w, self.h, self.n, self.flags = w, h, n, flags
        self.times = [f / 60.0 for f in range(n)]  # a clip at 60 frames per second
        self.views = orbit(n)
        self.scene, self.ids, self.centres = scene, IDS[:moved], np.ascontiguousarray(centres[:, :moved])
        self.tile, self.mo = planes(w, h, 1), planes(w, h, 1)
        self.tiles, self.albedo, self.nd, self.moments = (planes(w, h, n) for _ in range(4))

    def prepare(self):
        api.set_camera(None)
        api.set_scene(*self.scene)
        api.UpdateTest(self.times[0], 0, self.w, self.h, self.flags)


class Sequence(Mode):
    """(a): the only way before"""
    def __init__(self, *a):
        Mode.__init__(self, *a)
        self.scenes = []
        for j in range(self.n):
            s = self.scene[0].copy()
            for k, i in enumerate(self.ids):
                s["cx"][i], s["cy"][i], s["cz"][i] = self.centres[j, k]
            self.scenes.append(s)

    def clip(self):
        w, h = self.w, self.h
        for j in range(self.n):
            v = self.views[j]
            api.set_scene(self.scenes[j], self.scene[1])
            api.set_camera(v[0:3], v[3:6], float(v[6]), float(v[7]), float(v[8]))
            api.UpdateTest(0.0, j, w, h, self.flags)
            api.draw_device_moments(0.0, j, w, h, self.tiles[j].data_ptr(), self.moments[j].data_ptr(), self.flags,
                                    albedo_ptr=self.albedo[j].data_ptr(), normal_depth_ptr=self.nd[j].data_ptr())


class CameraClip(Mode):
    """(b): the library's own motion"""
    def clip(self):
        api.draw_device_camera_clip(self.times, self.views, 0, self.w, self.h, self.tile.data_ptr(), self.mo.data_ptr(), self.flags,
                                    images_ptr=self.tiles.data_ptr(), albedo_ptr=self.albedo.data_ptr(), normal_depth_ptr=self.nd.data_ptr(),
                                    frame_moments_ptr=self.moments.data_ptr())


class KeyframeClip(Mode):
    """(c): the caller's motion, one call per clip"""
    def clip(self):
        api.draw_device_keyframe_clip(self.views, self.ids, self.centres, 0, self.w, self.h, self.tile.data_ptr(), self.mo.data_ptr(),
                                      self.flags, images_ptr=self.tiles.data_ptr(), albedo_ptr=self.albedo.data_ptr(),
                                      normal_depth_ptr=self.nd.data_ptr(), frame_moments_ptr=self.moments.data_ptr())


def bracket(mode, reps):
    mode.prepare()
    api.synchronize()
    r0 = api.ray_counter_read()
    api.timer_begin()
    for _ in range(reps):
        mode.clip()
    ms = api.timer_end()
    return api.ray_counter_read() - r0, ms * 1e-3


def clip(name, w, h, spp, n, rounds, seconds):
    api.set_samples_per_pixel(spp)
    scene, centres = motion([f / 60.0 for f in range(n)], w, h)
    modes = {"a_set_scene_update_draw_moments": Sequence(w, h, n, 0, scene, centres, 8),
             "b_camera_clip_animate": CameraClip(w, h, n, ANIMATE, scene, centres, 0)}
    for k in (0, 2, 4, 8):
        modes["c_keyframe_clip_%d_moved" % k] = KeyframeClip(w, h, n, 0, scene, centres, k)
    torch.cuda.synchronize()
    reps = {}
    for m, mode in modes.items():  # warm-up (buffers, code objects), then how many clips make a bracket
        bracket(mode, 1)
        _, dt = bracket(mode, 2)
        reps[m] = max(1, math.ceil(seconds / (dt / 2)))
    ms, rate = {m: [] for m in modes}, {m: [] for m in modes}
    for r in range(rounds):
        for m, mode in modes.items():
            rays, dt = bracket(mode, reps[m])
            ms[m].append(dt / (reps[m] * n) * 1e3)
            rate[m].append(rays / dt / 1e9)
            print(json.dumps(dict(config=name, mode=m, round=r, clips=reps[m], seconds=round(dt, 3), ms_per_frame=round(ms[m][-1], 4),
                                  gray_s=round(rate[m][-1], 3))), flush=True)
    a, c8, b, c2 = (modes[m] for m in ("a_set_scene_update_draw_moments", "c_keyframe_clip_8_moved", "b_camera_clip_animate", "c_keyframe_clip_2_moved"))
    torch.cuda.synchronize()
    eq = lambda x, y: {k: bool(torch.equal(getattr(x, k).view(torch.int32), getattr(y, k).view(torch.int32))) for k in ("tiles", "albedo", "nd", "moments")}  # noqa: E731
    same = dict(a_and_c8=eq(a, c8), b_and_c2=eq(b, c2))
    kernel = {}
    for m, mode in modes.items():
        mode.prepare()
        api.kernel_timing_begin(4 + n)
        mode.clip()
        kernel[m] = api.kernel_timing_end()
    api.set_camera(None)
    api.set_scene(None)
    med_ms = {m: statistics.median(v) for m, v in ms.items()}
    med = {m: statistics.median(v) for m, v in rate.items()}
    slope = (med_ms["c_keyframe_clip_8_moved"] - med_ms["c_keyframe_clip_0_moved"]) / 8.0
    out = dict(config=name, w=w, h=h, spp=spp, frames_per_clip=n, rounds=rounds,
               median_ms_per_frame={m: round(v, 4) for m, v in med_ms.items()},
               range_ms_per_frame={m: [round(min(v), 4), round(max(v), 4)] for m, v in ms.items()},
               median_gray_s={m: round(v, 3) for m, v in med.items()},
               range_gray_s={m: [round(min(v), 3), round(max(v), 3)] for m, v in rate.items()},
               c_over_a_time={m: round(med_ms[m] / med_ms["a_set_scene_update_draw_moments"], 3) for m in modes if m.startswith("c_")},
               c2_over_b_time=round(med_ms["c_keyframe_clip_2_moved"] / med_ms["b_camera_clip_animate"], 3),
               ms_per_frame_per_moved_sphere=round(slope, 5), same_bytes=same,
               launches_per_call={m: k[1] for m, k in kernel.items()},
               kernel_ms_per_launch={m: round(k[0] / max(1, k[1]), 3) for m, k in kernel.items()}, pipeline=api.pipeline_info())
    print(json.dumps(out), flush=True)
    del modes, a, b, c2, c8
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.25, help="shortest bracket, as measured at warm-up")
    ap.add_argument("--frames", default="32,128", help="frames per clip, comma-separated")
    ap.add_argument("--only", default="", help="640x360 or 1280x720")
    args = ap.parse_args()
    api.InitializeTest()
    try:
        for w, h in ((640, 360), (1280, 720)):
            if args.only not in ("", "%dx%d" % (w, h)):
                continue
            for n in (int(x) for x in args.frames.split(",")):
                clip("%dx%dx4 %d frames" % (w, h, n), w, h, 4, n, args.rounds, args.seconds)
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
