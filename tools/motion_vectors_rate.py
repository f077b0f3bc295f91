"""A 32-frame keyframe clip's motion vectors, 640x360 and 1280x720 at 4 spp, in both forms (plain; object planes with api.motion_table
tables), two ways: (call) one motion_vectors_device call, and (passes) the 31 temporal_accumulate_[objects_]device calls a caller
issues on the same planes for frames 1 .. 31 -- the existing pass, whose steps 1-4 derive the same motion and which reads these planes
and four more per frame and writes four planes where the call writes one.  The passes are the yardstick, not a replacement: they
compute a blend the call does not.  Wall time of the host around as many clips as took at least --seconds at warm-up, each bracket
ended by tptSynchronize; the two ways alternate in one process, the one that goes first changes every round; the figures are medians
over the rounds with their range.  Prints one JSON line per (cell, way, round), one summary line per cell -- with whether the call's W
agrees with the passes' history lengths (W > 0 exactly where frame 1's pass, fed frame 0's as a first frame, finds a history) -- and the
table of profiles/motion_vectors/README.md.
    python3 tools/motion_vectors_rate.py [--rounds N] [--seconds S] [--frames N] [--only 640x360|1280x720]"""
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

MOVED = [2, 9]  # the keyframe clip's moved spheres (Lambert)
SPP = 4
TOL = {k: v for k, v in api.TEMPORAL_DEFAULTS.items() if k != "max_history"}


def orbit(n, step=0.5):
    a = np.radians(step * np.arange(n))
    v = np.zeros((n, 9), np.float32)
    v[:, 0], v[:, 1], v[:, 2] = 3.0 * np.sin(a), 2.0, 3.0 * np.cos(a)
    v[:, 6], v[:, 7], v[:, 8] = 60.0, 0.02, 3.0
    return v


def planes(w, h, n):
    return torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")


class Clip:
    """the planes of one tptDrawDeviceKeyframeClip call, and the buffers both ways write"""
    def __init__(self, w, h, n):
        self.w, self.h, self.n = w, h, n
        self.images, self.albedo, self.nd, self.moments = (planes(w, h, n) for _ in range(4))
        tile, mo = planes(w, h, 1), planes(w, h, 1)
        api.set_camera(None)
        api.set_scene(None)
        api.UpdateTest(0.0, 0, w, h, 0)
        spheres = api.GetSceneDesc()[0].copy()
        centres = np.zeros((n, len(MOVED), 3), np.float32)
        for j in range(n):
            for k, i in enumerate(MOVED):
                centres[j, k] = (spheres["cx"][i] + np.float32(0.05) * j * (1 - 2 * k), spheres["cy"][i], spheres["cz"][i])
        self.objects = torch.zeros((n, h, w), dtype=torch.int32, device="cuda")
        self.cams = api.draw_device_keyframe_clip(orbit(n), MOVED, centres, 0, w, h, tile.data_ptr(), mo.data_ptr(), 0,
                                                  images_ptr=self.images.data_ptr(), albedo_ptr=self.albedo.data_ptr(),
                                                  normal_depth_ptr=self.nd.data_ptr(), frame_moments_ptr=self.moments.data_ptr(),
                                                  objects_ptr=self.objects.data_ptr())
        tables = [np.zeros((len(spheres), 4), np.float32)]
        for j in range(1, n):
            a, b = spheres.copy(), spheres.copy()
            for k, i in enumerate(MOVED):
                a["cx"][i], b["cx"][i] = centres[j - 1, k, 0], centres[j, k, 0]
            tables.append(api.motion_table(a, b))
        self.motion = torch.from_numpy(np.stack(tables)).cuda()
        self.n_objects = len(spheres)
        api.synchronize()
        api.set_camera(None)
        api.set_scene(None)
        self.t = torch.zeros((2, 4, h, w, 4), dtype=torch.float32, device="cuda")  # the passes' outputs of even and odd frames
        self.flow = planes(w, h, n)


def passes(c, form):
    """tptTemporalAccumulate[Objects]Device for frames 1 .. n-1, each on the frame before as traced: 31 launches for 32 frames"""
    w, h = c.w, c.h
    for j in range(1, c.n):
        cur = [s[j].data_ptr() for s in (c.images, c.albedo, c.nd, c.moments)]
        before = [s[j - 1].data_ptr() for s in (c.images, c.albedo, c.nd, c.moments)]
        o = [c.t[j & 1, k].data_ptr() for k in range(4)]
        if form == "objects":
            api.temporal_accumulate_objects_device(w, h, c.cams[j], *cur, c.objects[j].data_ptr(), *o,
                                                   prev=(c.cams[j - 1], *before, c.objects[j - 1].data_ptr()),
                                                   motion_ptr=c.motion[j].data_ptr(), n_objects=c.n_objects, max_history=2.0)
        else:
            api.temporal_accumulate_device(w, h, c.cams[j], *cur, *o, prev=(c.cams[j - 1], *before), max_history=2.0)


def call(c, form):
    """one tptMotionVectorsDevice call"""
    kw = {}
    if form == "objects":
        kw.update(objects_ptr=c.objects.data_ptr(), motion_ptr=c.motion.data_ptr(), n_objects=c.n_objects)
    api.motion_vectors_device(c.w, c.h, c.n, c.albedo.data_ptr(), c.nd.data_ptr(), c.flow.data_ptr(), c.cams, **kw, **TOL)


WAYS = {"passes": passes, "call": call}


def bracket(way, c, form, reps):
    api.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        WAYS[way](c, form)
    api.synchronize()
    return time.perf_counter() - t0


def agrees(c, form):
    """frame 0 through the pass as a first frame, frame 1 with maxHistory = 2: its history length is 2 exactly where the call's W > 0"""
    w, h = c.w, c.h
    cur = lambda j: [s[j].data_ptr() for s in (c.images, c.albedo, c.nd, c.moments)]  # noqa: E731
    t0, t1 = ([c.t[i, k].data_ptr() for k in range(4)] for i in range(2))
    if form == "objects":
        api.temporal_accumulate_objects_device(w, h, c.cams[0], *cur(0), c.objects[0].data_ptr(), *t0, max_history=2.0)
        api.temporal_accumulate_objects_device(w, h, c.cams[1], *cur(1), c.objects[1].data_ptr(), *t1,
                                               prev=(c.cams[0], t0[0], t0[1], cur(0)[2], t0[2], c.objects[0].data_ptr()),
                                               motion_ptr=c.motion[1].data_ptr(), n_objects=c.n_objects, max_history=2.0)
    else:
        api.temporal_accumulate_device(w, h, c.cams[0], *cur(0), *t0, max_history=2.0)
        api.temporal_accumulate_device(w, h, c.cams[1], *cur(1), *t1, prev=(c.cams[0], t0[0], t0[1], cur(0)[2], t0[2]), max_history=2.0)
    call(c, form)
    api.synchronize()
    torch.cuda.synchronize()
    return bool(torch.equal(c.t[1, 2][..., 3] == 2, c.flow[1][..., 3] > 0))


def cell(name, c, form, rounds, seconds):
    reps = {}
    for way in WAYS:  # warm-up (buffers, code objects, the library's table), then how many clips make a bracket
        bracket(way, c, form, 1)
        reps[way] = max(1, math.ceil(seconds / (bracket(way, c, form, 4) / 4)))
    ms = {way: [] for way in WAYS}
    for r in range(rounds):
        for way in (("passes", "call") if r % 2 == 0 else ("call", "passes")):
            dt = bracket(way, c, form, reps[way])
            ms[way].append(dt / reps[way] * 1e3)
            print(json.dumps(dict(config=name, form=form, way=way, round=r, clips=reps[way], seconds=round(dt, 4),
                                  ms_per_clip=round(ms[way][-1], 4))), flush=True)
    med = {way: statistics.median(v) for way, v in ms.items()}
    out = dict(config=name, form=form, frames_per_clip=c.n, rounds=rounds, median_ms_per_clip={k: round(v, 4) for k, v in med.items()},
               range_ms_per_clip={k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
               median_us_per_frame={k: round(v / c.n * 1e3, 2) for k, v in med.items()},
               call_over_passes_time=round(med["call"] / med["passes"], 3), weight_agrees=agrees(c, form))
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
            c = Clip(w, h, args.frames)
            for form in ("plain", "objects"):
                rows.append(cell("%dx%dx%d %d frames" % (w, h, SPP, args.frames), c, form, args.rounds, args.seconds))
            del c
            torch.cuda.empty_cache()
    finally:
        api.ShutdownTest()
    print("| size | form | %d passes, ms per clip (range) | call, ms per clip (range) | call / passes | W agrees |" % (args.frames - 1))
    print("|---|---|---|---|---|---|")
    for r in rows:
        m, g = r["median_ms_per_clip"], r["range_ms_per_clip"]
        print("| %s | %s | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.2f | %s |" % (
            r["config"], r["form"], m["passes"], g["passes"][0], g["passes"][1], m["call"], g["call"][0], g["call"][1],
            r["call_over_passes_time"], "yes" if r["weight_agrees"] else "NO"))


if __name__ == "__main__":
    main()
