"""A 32-frame clip through the denoising chain, 640x360 and 1280x720 at 4 spp, at the defaults (5 iterations, both guides, demodulated),
in three modes: the filter alone on every frame (spatial-only), the plain temporal pass in front of it (a tptDrawDeviceCameraClip
clip, 0.5 degrees of orbit per frame over the animated scene), and the object-following pass (a tptDrawDeviceKeyframeClip clip, two
spheres moved by the caller, api.motion_table tables with a cap of 2 on the metal and glass spheres).  Each mode two ways: (chain) the
per-frame entry points through the Python binding -- temporal_accumulate_[objects_]device and denoise_device_variance per frame, the
only way before, and unchanged code -- and (call) one denoise_clip_device call.  Wall time of the host around as many clips as took at
least --seconds at warm-up, each bracket ended by tptSynchronize; the two ways alternate, the one that goes first changes every
round; the figures are medians over the rounds with their range.  Prints one JSON line per (cell, way, round), one summary line per
cell -- with whether both ways wrote the same bytes -- and the table of profiles/clip_denoise/README.md.
    python3 tools/clip_denoise_rate.py [--rounds N] [--seconds S] [--frames N] [--only 640x360|1280x720]"""
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

ANIMATE = 1  # kFlagAnimate (without kFlagProgressive: every frame its own)
MOVED = [2, 9]  # the keyframe clip's moved spheres (Lambert)
SPP = 4


def orbit(n, step=0.5):
    a = np.radians(step * np.arange(n))
    v = np.zeros((n, 9), np.float32)
    v[:, 0], v[:, 1], v[:, 2] = 3.0 * np.sin(a), 2.0, 3.0 * np.cos(a)
    v[:, 6], v[:, 7], v[:, 8] = 60.0, 0.02, 3.0
    return v


def planes(w, h, n):
    return torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")


class Clip:
    """the planes of one clip draw, and the buffers both ways write"""
    def __init__(self, w, h, n, keyframes):
        self.w, self.h, self.n = w, h, n
        self.images, self.albedo, self.nd, self.moments = (planes(w, h, n) for _ in range(4))
        tile, mo = planes(w, h, 1), planes(w, h, 1)
        outs = dict(images_ptr=self.images.data_ptr(), albedo_ptr=self.albedo.data_ptr(), normal_depth_ptr=self.nd.data_ptr(),
                    frame_moments_ptr=self.moments.data_ptr())
        api.set_camera(None)
        api.set_scene(None)
        self.objects = self.motion = None
        self.n_objects = 0
        if keyframes:
            api.UpdateTest(0.0, 0, w, h, 0)
            spheres, mats = (a.copy() for a in api.GetSceneDesc()[:2])
            centres = np.zeros((n, len(MOVED), 3), np.float32)
            for j in range(n):
                for k, i in enumerate(MOVED):
                    centres[j, k] = (spheres["cx"][i] + np.float32(0.05) * j * (1 - 2 * k), spheres["cy"][i], spheres["cz"][i])
            self.objects = torch.zeros((n, h, w), dtype=torch.int32, device="cuda")
            self.cams = api.draw_device_keyframe_clip(orbit(n), MOVED, centres, 0, w, h, tile.data_ptr(), mo.data_ptr(), 0,
                                                      objects_ptr=self.objects.data_ptr(), **outs)
            caps = np.where(mats["type"] != 0, 2.0, 0.0).astype(np.float32)
            tables = [np.zeros((len(spheres), 4), np.float32)]
            for j in range(1, n):
                a, b = spheres.copy(), spheres.copy()
                for k, i in enumerate(MOVED):
                    a["cx"][i], b["cx"][i] = centres[j - 1, k, 0], centres[j, k, 0]
                tables.append(api.motion_table(a, b, caps))
            self.motion = torch.from_numpy(np.stack(tables)).cuda()
            self.n_objects = len(spheres)
        else:
            times = [f / 60.0 for f in range(n)]
            api.UpdateTest(times[0], 0, w, h, ANIMATE)
            self.cams = api.draw_device_camera_clip(times, orbit(n), 0, w, h, tile.data_ptr(), mo.data_ptr(), ANIMATE, **outs)
        api.synchronize()
        api.set_camera(None)
        api.set_scene(None)
        self.t = torch.zeros((2, 4, h, w, 4), dtype=torch.float32, device="cuda")  # the chain's T of even and odd frames
        self.out = {"chain": planes(w, h, n), "call": planes(w, h, n)}


def chain(c, mode):
    """the per-frame entry points: what a caller issued before"""
    w, h = c.w, c.h
    prev = None
    for j in range(c.n):
        cur = [s[j].data_ptr() for s in (c.images, c.albedo, c.nd, c.moments)]
        out = c.out["chain"][j].data_ptr()
        if mode == "spatial":
            api.denoise_device_variance(w, h, cur[0], cur[3], float(SPP), out, albedo_ptr=cur[1], normal_depth_ptr=cur[2])
            continue
        o = [c.t[j & 1, k].data_ptr() for k in range(4)]
        if mode == "objects":
            table = prev is not None
            api.temporal_accumulate_objects_device(w, h, c.cams[j], *cur, c.objects[j].data_ptr(), *o, prev=prev,
                                                   motion_ptr=c.motion[j].data_ptr() if table else None,
                                                   n_objects=c.n_objects if table else 0)
            prev = (c.cams[j], o[0], o[1], cur[2], o[2], c.objects[j].data_ptr())
        else:
            api.temporal_accumulate_device(w, h, c.cams[j], *cur, *o, prev=prev)
            prev = (c.cams[j], o[0], o[1], cur[2], o[2])
        api.denoise_device_variance(w, h, o[0], o[3], float(SPP), out, albedo_ptr=o[1], normal_depth_ptr=cur[2])


def call(c, mode):
    """one tptDenoiseClipDevice call"""
    kw = dict(albedo_ptr=c.albedo.data_ptr(), normal_depth_ptr=c.nd.data_ptr())
    if mode == "spatial":
        kw.update(spatial_only=True)
    else:
        kw.update(cameras=c.cams)
    if mode == "objects":
        kw.update(objects_ptr=c.objects.data_ptr(), motion_ptr=c.motion.data_ptr(), n_objects=c.n_objects)
    api.denoise_clip_device(c.w, c.h, c.n, c.images.data_ptr(), c.moments.data_ptr(), c.out["call"].data_ptr(), float(SPP), **kw)


WAYS = {"chain": chain, "call": call}


def bracket(way, c, mode, reps):
    api.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        WAYS[way](c, mode)
    api.synchronize()
    return time.perf_counter() - t0


def cell(name, c, mode, rounds, seconds):
    reps = {}
    for way in WAYS:  # warm-up (buffers, code objects, the library's staging), then how many clips make a bracket
        bracket(way, c, mode, 1)
        reps[way] = max(1, math.ceil(seconds / (bracket(way, c, mode, 4) / 4)))
    ms = {way: [] for way in WAYS}
    for r in range(rounds):
        for way in (("chain", "call") if r % 2 == 0 else ("call", "chain")):
            dt = bracket(way, c, mode, reps[way])
            ms[way].append(dt / reps[way] * 1e3)
            print(json.dumps(dict(config=name, mode=mode, way=way, round=r, clips=reps[way], seconds=round(dt, 4),
                                  ms_per_clip=round(ms[way][-1], 4))), flush=True)
    torch.cuda.synchronize()
    same = bool(torch.equal(c.out["chain"].view(torch.int32), c.out["call"].view(torch.int32)))
    med = {way: statistics.median(v) for way, v in ms.items()}
    out = dict(config=name, mode=mode, frames_per_clip=c.n, rounds=rounds, median_ms_per_clip={k: round(v, 4) for k, v in med.items()},
               range_ms_per_clip={k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
               median_us_per_frame={k: round(v / c.n * 1e3, 2) for k, v in med.items()},
               call_over_chain_time=round(med["call"] / med["chain"], 3), same_bytes=same)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.25, help="shortest bracket, as measured at warm-up")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--only", default="", help="640x360 or 1280x720")
    args = ap.parse_args()
    api.InitializeTest()
    rows = []
    try:
        api.set_samples_per_pixel(SPP)
        for w, h in ((640, 360), (1280, 720)):
            if args.only not in ("", "%dx%d" % (w, h)):
                continue
            for keyframes, modes in ((False, ("spatial", "temporal")), (True, ("objects",))):
                c = Clip(w, h, args.frames, keyframes)
                for mode in modes:
                    rows.append(cell("%dx%dx%d %d frames" % (w, h, SPP, args.frames), c, mode, args.rounds, args.seconds))
                del c
                torch.cuda.empty_cache()
    finally:
        api.ShutdownTest()
    print("| size | mode | chain, ms per clip (range) | call, ms per clip (range) | call / chain | same bytes |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        m, g = r["median_ms_per_clip"], r["range_ms_per_clip"]
        print("| %s | %s | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.2f | %s |" % (
            r["config"], r["mode"], m["chain"], g["chain"][0], g["chain"][1], m["call"], g["call"][0], g["call"][1],
            r["call_over_chain_time"], "yes" if r["same_bytes"] else "NO"))


if __name__ == "__main__":
    main()
